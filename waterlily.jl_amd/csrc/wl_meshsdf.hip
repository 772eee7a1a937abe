// Distance fields from closed meshes (include/wlhip.h wl_sdf_lattice_from_mesh): the exact signed distance from every sample of a lattice to a closed
// triangle surface (2-D: closed polygons of segments).  An all-pairs search with culling — compute-bound, nothing like the streaming kernels of this library:
//   one wave owns a brick of 4×4×4 samples (2-D: 4×16), four waves a workgroup; the workgroup walks the elements in chunks of 256 staged in LDS (vertices and
//   a bounding sphere each);
//   sweep 1, per wave, over the spheres alone: Ub = min_t(|c_brick − c_t| + r_t) + r_brick bounds the distance of every sample of the brick from above;
//   sweep 2: element t is a candidate of the brick when |c_brick − c_t| − r_t − r_brick ≤ Ub (with a slack that covers the rounding of either side); the
//   wave ballots 64 elements at a time and walks the set bits of the ballot in ascending order — every lane then reads the same LDS address (a broadcast) and
//   runs the exact closest-point walk (Ericson, Real-Time Collision Detection §5.1.5) for its own sample, the running minimum in registers.
// The candidates of a brick are visited in ascending element index with a strict <, exactly as the brute-force flag visits all of them: the element that wins
// under brute force is the first that attains the computed minimum, it is a candidate (its true distance is at most Ub), so both forms store the same bits.
// No list is kept (the ballot is the list, 64 entries at a time, consumed at once: any candidate count works), no atomics, nothing between workgroups.
// The sign: (p − q)·n with the angle-weighted pseudonormal of the winning feature (Bærentzen & Aanæs 2005), gathered once per sample after the search.
#include <chrono>
#include <cmath>
#include <string>
#include <unordered_map>

#include "wl_meshsdf.hpp"

namespace {
constexpr int MS_CHUNK = 256;
struct MsArgs {
  const float* elem; const float4* sph; const float* nrm; float* a; unsigned long long* pairs;
  int32_t ne; int32_t n[3]; int32_t nb[3]; long nbricks;
  float c[3]; float s; float rb; float slack; int brute;
  const float* wtab; float* w;      // VEL: the vertex velocities per element (ne×D×D, vertex-major like elem) and the D component planes they are extended into
  float band;                       // BAND: the samples are clipped to ±band; a brick wholly beyond it is not searched (last: the offsets above stay what they were)
};
constexpr unsigned long long MS_SKIPPED = 1ull << 63;    // BAND: set in a brick's `pairs` entry when the brick was skipped (one sign search instead of sweep 2)
unsigned long long g_ms_tested = 0, g_ms_total = 0;      // wl_meshsdf_last_pairs
unsigned long long g_ms_searched = 0, g_ms_skipped = 0;  // wl_meshsdf_last_bricks
double g_ms_ms[4] = {0, 0, 0, 0};                        // wl_meshsdf_last_times
int g_ms_timed = 0;
}  // namespace

#pragma clang fp contract(off)
namespace {
// the closest point q of element e (vertices in LDS) to p: r = p − q, d² = |r|², reg = the region of the walk (the row of the pseudonormal table).
// VEL: also the barycentric pair (bv, bw) of q = A + bv·(B − A) + bw·(C − A), read off the region the walk decides — never solved for again
template <bool VEL>
__device__ __forceinline__ void ms_pair(const float* e, const float (&p)[3], float& d2, int& reg, float (&r)[3], float& bv, float& bw) {
  const float a[3] = {e[0], e[1], e[2]}, b[3] = {e[3], e[4], e[5]}, c[3] = {e[6], e[7], e[8]};
  float ab[3], ac[3], ap[3], q[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; ap[k] = p[k] - a[k]; }
  const float d1 = (ab[0] * ap[0] + ab[1] * ap[1]) + ab[2] * ap[2];
  const float d2_ = (ac[0] * ap[0] + ac[1] * ap[1]) + ac[2] * ap[2];
  const float bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
  const float d3 = (ab[0] * bp[0] + ab[1] * bp[1]) + ab[2] * bp[2];
  const float d4 = (ac[0] * bp[0] + ac[1] * bp[1]) + ac[2] * bp[2];
  const float cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
  const float d5 = (ab[0] * cp[0] + ab[1] * cp[1]) + ab[2] * cp[2];
  const float d6 = (ac[0] * cp[0] + ac[1] * cp[1]) + ac[2] * cp[2];
  const float vc = d1 * d4 - d3 * d2_, vb = d5 * d2_ - d1 * d6, va = d3 * d6 - d5 * d4;
  if (d1 <= 0.f && d2_ <= 0.f) {                                            // vertex A
    reg = 4;
    if constexpr (VEL) { bv = 0.f; bw = 0.f; }
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = a[k];
  } else if (d3 >= 0.f && d4 <= d3) {                                       // vertex B
    reg = 5;
    if constexpr (VEL) { bv = 1.f; bw = 0.f; }
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = b[k];
  } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {                         // edge AB
    reg = 1;
    const float v = d1 / (d1 - d3);
    if constexpr (VEL) { bv = v; bw = 0.f; }
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = a[k] + v * ab[k];
  } else if (d6 >= 0.f && d5 <= d6) {                                       // vertex C
    reg = 6;
    if constexpr (VEL) { bv = 0.f; bw = 1.f; }
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = c[k];
  } else if (vb <= 0.f && d2_ >= 0.f && d6 <= 0.f) {                        // edge CA
    reg = 3;
    const float w = d2_ / (d2_ - d6);
    if constexpr (VEL) { bv = 0.f; bw = w; }
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = a[k] + w * ac[k];
  } else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {           // edge BC
    reg = 2;
    const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
    if constexpr (VEL) { bv = 1.f - w; bw = w; }
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = b[k] + w * (c[k] - b[k]);
  } else {                                                                  // the face
    reg = 0;
    const float den = 1.f / ((va + vb) + vc);
    const float v = vb * den, w = vc * den;
    if constexpr (VEL) { bv = v; bw = w; }
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = (a[k] + ab[k] * v) + ac[k] * w;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) r[k] = p[k] - q[k];
  d2 = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
}
template <bool VEL>
__device__ __forceinline__ void ms_pair(const float* e, const float (&p)[2], float& d2, int& reg, float (&r)[2], float& bv, float& bw) {
  const float a[2] = {e[0], e[1]}, b[2] = {e[2], e[3]};
  const float ab[2] = {b[0] - a[0], b[1] - a[1]}, ap[2] = {p[0] - a[0], p[1] - a[1]};
  const float t = ab[0] * ap[0] + ab[1] * ap[1];
  const float den = ab[0] * ab[0] + ab[1] * ab[1];
  float q[2];
  if (t <= 0.f) { reg = 1; q[0] = a[0]; q[1] = a[1]; if constexpr (VEL) bv = 0.f; }                      // vertex A
  else if (t >= den) { reg = 2; q[0] = b[0]; q[1] = b[1]; if constexpr (VEL) bv = 1.f; }                 // vertex B
  else { reg = 0; const float v = t / den; q[0] = a[0] + v * ab[0]; q[1] = a[1] + v * ab[1]; if constexpr (VEL) bv = v; }
  if constexpr (VEL) bw = 0.f;
  r[0] = p[0] - q[0]; r[1] = p[1] - q[1];
  d2 = r[0] * r[0] + r[1] * r[1];
}

// BAND (a lattice made with a band b, wlhip.h band-limited baking): every sample stores clip(d, −b, +b).  Sweep 1 also forms the brick's lower bound
// Lb = min_t(|c_b − c_t| − r_t) − r_b; a brick with Lb above b (plus the slack of the threshold, on the safe side) is FAR: it does not meet the surface, so
// its samples share one sign and all of them are clipped.  A far wave finds that sign by searching for its first sample alone, in parallel over the
// elements: each lane walks its own elements in ascending index with a strict <, a wave reduction then takes the smallest d² and, on equal d², the smallest
// index — the winner of the serial walk, with its bits.  Far and near waves of a workgroup walk the same chunk loop: the barriers are those of BAND = false.
template <int D, bool VEL, bool BAND>
__global__ __launch_bounds__(256) void k_meshsdf(const MsArgs A) {
  constexpr int NE = D * D, NR = D == 3 ? 7 : 3;
  constexpr int EXT[3] = {4, D == 3 ? 4 : 16, D == 3 ? 4 : 1};
  __shared__ float s_e[MS_CHUNK * NE];
  __shared__ float4 s_s[MS_CHUNK];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long brick = (long)blockIdx.x * 4 + wv;
  const bool wave_on = brick < A.nbricks;                  // a whole wave: the last workgroup may own fewer than four bricks
  int i[3] = {0, 0, 0}, i0[3] = {0, 0, 0};
  {
    long q = wave_on ? brick : 0;
    i0[0] = (int)(q % A.nb[0]) * EXT[0]; q /= A.nb[0];
    i0[1] = (int)(q % A.nb[1]) * EXT[1]; q /= A.nb[1];
    i0[2] = (int)q * EXT[2];
    i[0] = i0[0] + (lane & 3);
    i[1] = i0[1] + (D == 3 ? ((lane >> 2) & 3) : (lane >> 2));
    i[2] = i0[2] + (D == 3 ? (lane >> 4) : 0);
  }
  bool live = wave_on;                                     // ragged bricks: the lanes past the lattice search like the others and store nothing
  float p[D], cb[D];
#pragma unroll
  for (int d = 0; d < D; d++) {
    live = live && i[d] < A.n[d];
    p[d] = A.c[d] + A.s * ((float)i[d] - 0.5f);
    cb[d] = A.c[d] + A.s * (((float)i0[d] + 0.5f * (float)(EXT[d] - 1)) - 0.5f);
  }
  // sweep 1: the upper bound of the brick, over the spheres alone (global memory, every lane its own elements)
  float thresh = INFINITY;
  bool far = false;                                        // BAND: the whole brick lies beyond the band (the same value in every lane)
  float p0[D];                                             // BAND: the brick's first sample, lane 0's p in every lane
  if (!A.brute && wave_on) {
    float m = INFINITY, lo = INFINITY;
    for (int t = lane; t < A.ne; t += 64) {
      const float4 q = A.sph[t];
      float dd = (q.x - cb[0]) * (q.x - cb[0]) + (q.y - cb[1]) * (q.y - cb[1]);
      if (D == 3) dd = dd + (q.z - cb[D - 1]) * (q.z - cb[D - 1]);
      m = fminf(m, sqrtf(dd) + q.w);
      if constexpr (BAND) lo = fminf(lo, sqrtf(dd) - q.w);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o, 64));
    const float ub = m + A.rb;
    thresh = ub + (ub * 1e-4f + A.slack);
    if constexpr (BAND) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) lo = fminf(lo, __shfl_xor(lo, o, 64));
      far = lo - A.rb > A.band + (A.band * 1e-4f + A.slack);
      if (far) {                                           // the first sample's own bound (r_b = 0): what the sign search culls with
#pragma unroll
        for (int d = 0; d < D; d++) p0[d] = A.c[d] + A.s * ((float)i0[d] - 0.5f);
        float mp = INFINITY;
        for (int t = lane; t < A.ne; t += 64) {
          const float4 q = A.sph[t];
          float dd = (q.x - p0[0]) * (q.x - p0[0]) + (q.y - p0[1]) * (q.y - p0[1]);
          if (D == 3) dd = dd + (q.z - p0[D - 1]) * (q.z - p0[D - 1]);
          mp = fminf(mp, sqrtf(dd) + q.w);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mp = fminf(mp, __shfl_xor(mp, o, 64));
        thresh = mp + (mp * 1e-4f + A.slack);
      }
    }
  }
  // sweep 2: the candidates of each staged chunk, exactly
  float best = INFINITY, br[D];
  int bt = 0, breg = 0;
  float bbv = 0.f, bbw = 0.f;                              // VEL: the winner's barycentric pair
#pragma unroll
  for (int d = 0; d < D; d++) br[d] = 0.f;
  unsigned long long ntest = 0;
  for (int base = 0; base < A.ne; base += MS_CHUNK) {
    __syncthreads();                                       // the chunk before this one has been consumed by all four waves
    const int t = base + (int)threadIdx.x;
    if (t < A.ne) {
#pragma unroll
      for (int k = 0; k < NE; k++) s_e[threadIdx.x * NE + k] = A.elem[(size_t)t * NE + k];
      s_s[threadIdx.x] = A.sph[t];
    }
    __syncthreads();
    if (!wave_on) continue;                                // (no barrier below: the loop bounds are the same for every wave)
    const int cnt = min(MS_CHUNK, A.ne - base);
    if constexpr (BAND) {
      if (far) {                                           // the sign search: one point, every lane its own element of each 64-group
        for (int k = 0; k < cnt; k += 64) {
          const int j = k + lane;
          bool cand = j < cnt;
          if (cand) {
            const float4 q = s_s[j];
            float dd = (q.x - p0[0]) * (q.x - p0[0]) + (q.y - p0[1]) * (q.y - p0[1]);
            if (D == 3) dd = dd + (q.z - p0[D - 1]) * (q.z - p0[D - 1]);
            cand = sqrtf(dd) - q.w <= thresh;
          }
          const unsigned long long mask = __ballot(cand);
          if (!mask) continue;                             // a 64-group without a candidate is skipped as a whole
          ntest += (unsigned long long)__popcll(mask);
          if (cand) {
            float d2, r[D], pv = 0.f, pw = 0.f; int reg;
            ms_pair<false>(&s_e[j * NE], p0, d2, reg, r, pv, pw);
            if (d2 < best) {
              best = d2; bt = base + j; breg = reg;
#pragma unroll
              for (int d = 0; d < D; d++) br[d] = r[d];
            }
          }
        }
        continue;
      }
    }
    for (int k = 0; k < cnt; k += 64) {
      const int j = k + lane;
      bool cand = j < cnt;
      if (cand && !A.brute) {
        const float4 q = s_s[j];
        float dd = (q.x - cb[0]) * (q.x - cb[0]) + (q.y - cb[1]) * (q.y - cb[1]);
        if (D == 3) dd = dd + (q.z - cb[D - 1]) * (q.z - cb[D - 1]);
        cand = (sqrtf(dd) - q.w) - A.rb <= thresh;
      }
      unsigned long long mask = __ballot(cand);           // wave64: one bit per lane, the same value in every lane
      ntest += (unsigned long long)__popcll(mask);
      while (mask) {
        const int jj = k + __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        float d2, r[D], pv = 0.f, pw = 0.f; int reg;
        ms_pair<VEL>(&s_e[jj * NE], p, d2, reg, r, pv, pw);
        if (d2 < best) {
          best = d2; bt = base + jj; breg = reg;
          if constexpr (VEL) { bbv = pv; bbw = pw; }
#pragma unroll
          for (int d = 0; d < D; d++) br[d] = r[d];
        }
      }
    }
  }
  if constexpr (BAND) {
    if (far) {
      // the first of the smallest d² over the lanes: (d², index) in lexicographic order — an element belongs to one lane only (index ≡ lane mod 64)
      float md = best; int mt = best < INFINITY ? bt : 0x7fffffff;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float od = __shfl_xor(md, o, 64); const int ot = __shfl_xor(mt, o, 64);
        if (od < md || (od == md && ot < mt)) { md = od; mt = ot; }
      }
      const unsigned long long wm = __ballot(best == md && bt == mt);
      const int src = wm ? __ffsll((long long)wm) - 1 : 0;
      if (!wm) mt = 0;                                     // (guard: the element that attains the point's bound is always a candidate)
      const int wreg = __shfl(breg, src, 64);
      float wr[D];
#pragma unroll
      for (int d = 0; d < D; d++) wr[d] = __shfl(br[d], src, 64);
      if (lane == 0) A.pairs[brick] = ntest | MS_SKIPPED;
      if (live) {
        const float* nn = A.nrm + ((size_t)mt * NR + wreg) * D;
        float sg = wr[0] * nn[0] + wr[1] * nn[1];
        if (D == 3) sg = sg + wr[D - 1] * nn[D - 1];
        const size_t o = (size_t)i[0] + (size_t)A.n[0] * ((size_t)i[1] + (size_t)A.n[1] * (size_t)i[2]);
        A.a[o] = sg < 0.f ? -A.band : A.band;
        if constexpr (VEL) {
          const size_t plane = (size_t)A.n[0] * (size_t)A.n[1] * (size_t)A.n[2];
#pragma unroll
          for (int c = 0; c < D; c++) A.w[(size_t)c * plane + o] = 0.f;
        }
      }
      return;                                              // (no barrier below)
    }
  }
  const unsigned long long nlive = (unsigned long long)__popcll(__ballot(live));
  if (wave_on && lane == 0) A.pairs[brick] = ntest * nlive;
  if (live) {
    const float* nn = A.nrm + ((size_t)bt * NR + breg) * D;
    float sg = br[0] * nn[0] + br[1] * nn[1];
    if (D == 3) sg = sg + br[D - 1] * nn[D - 1];
    const float d = sqrtf(best);
    const size_t o = (size_t)i[0] + (size_t)A.n[0] * ((size_t)i[1] + (size_t)A.n[1] * (size_t)i[2]);
    if constexpr (BAND) {
      if (d > A.band) {                                    // the clip: ±band with the sign of the full value, no velocity beyond the band
        A.a[o] = sg < 0.f ? -A.band : A.band;
        if constexpr (VEL) {
          const size_t plane = (size_t)A.n[0] * (size_t)A.n[1] * (size_t)A.n[2];
#pragma unroll
          for (int c = 0; c < D; c++) A.w[(size_t)c * plane + o] = 0.f;
        }
        return;
      }
    }
    A.a[o] = sg < 0.f ? -d : d;                            // d = 0 has p = q, sg = ±0: +0 is stored
    if constexpr (VEL) {                                   // the closest-point extension of the vertex velocities: W = wa + v·(wb − wa) + w·(wc − wa), gathered once
      const float* wt = A.wtab + (size_t)bt * NE;
      const size_t plane = (size_t)A.n[0] * (size_t)A.n[1] * (size_t)A.n[2];
#pragma unroll
      for (int c = 0; c < D; c++) {
        const float wa = wt[c], wb = wt[D + c];
        float W = wa + bbv * (wb - wa);
        if (D == 3) W = W + bbw * (wt[2 * D + c] - wa);
        A.w[(size_t)c * plane + o] = W;
      }
    }
  }
}
}  // namespace

namespace {
struct V3 { double x, y, z; };
inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 mul(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline double norm(V3 a) { return std::sqrt(dot(a, a)); }
// a / |a|, or `fallback` where the sum cancels (a fold of 180°)
inline V3 unit_or(V3 a, V3 fallback) { const double n = norm(a); return (n > 0 && std::isfinite(1.0 / n)) ? mul(a, 1.0 / n) : fallback; }
inline uint64_t ekey(int32_t i, int32_t j) { return ((uint64_t)(uint32_t)i << 32) | (uint32_t)j; }
// the smallest sphere around k points (2 or 3): the midpoint sphere of an edge if it holds the third point, else the circumsphere
void bounding_sphere(const V3* p, int k, V3* c, double* r) {
  double best = INFINITY;
  for (int a = 0; a < k; a++)
    for (int b = a + 1; b < k; b++) {
      const V3 m = mul(add(p[a], p[b]), 0.5);
      double rr = 0;
      for (int q = 0; q < k; q++) rr = std::fmax(rr, norm(sub(p[q], m)));
      if (rr <= 0.5 * norm(sub(p[a], p[b])) * (1 + 1e-12) && rr < best) { best = rr; *c = m; }
    }
  if (!(best < INFINITY)) {                                // an acute triangle: the circumcentre
    const V3 ab = sub(p[1], p[0]), ac = sub(p[2], p[0]), n = cross(ab, ac);
    const V3 m = add(p[0], mul(add(mul(cross(n, ab), dot(ac, ac)), mul(cross(ac, n), dot(ab, ab))), 0.5 / dot(n, n)));
    *c = m; best = 0;
    for (int q = 0; q < k; q++) best = std::fmax(best, norm(sub(p[q], m)));
  }
  *r = best;
}
}  // namespace

namespace wl {
// One body for both entry points, so that everything that is rounded comes from the same statements in the same order.  topo NULL: the call of a lattice's
// creation — every refusal in the documented order, the adjacency built (and left in out->adj).  topo given (the adjacency kept since creation, for the same
// e): the index checks, the edge map and the 2-D in/out tables are skipped — they depend on the connectivity alone and have passed.
static int prepare_tables(int D, const float* v, int32_t nv, const int32_t* e, int32_t ne, const std::vector<int32_t>* topo, MeshTables* out, const char* who) {
  const std::string F = std::string(who) + ": ";
  if (D == 3 ? (nv < 4 || ne < 4) : (nv < 3 || ne < 3)) {
    wl_set_error(F + (D == 3 ? "a closed surface has at least 4 vertices and 4 triangles" : "a closed polygon has at least 3 vertices and 3 segments"));
    return WL_EINVAL;
  }
  double scale = 0;
  for (size_t q = 0; q < (size_t)nv * D; q++) {
    if (!std::isfinite(v[q])) { wl_set_error(F + "vertex " + std::to_string(q / D) + " is not finite"); return WL_EINVAL; }
    scale = std::fmax(scale, std::fabs((double)v[q]));
  }
  for (size_t q = 0; !topo && q < (size_t)ne * D; q++)
    if (e[q] < 0 || e[q] >= nv) { wl_set_error(F + "element " + std::to_string(q / D) + " names index " + std::to_string(e[q]) + " outside [0, nv)"); return WL_EINVAL; }
  auto P = [&](int32_t i) { return V3{v[(size_t)i * D], v[(size_t)i * D + 1], D == 3 ? v[(size_t)i * D + 2] : 0.0}; };
  const int NR = D == 3 ? 7 : 3;
  std::vector<V3> nf(ne);                                   // unit face (edge) normals
  for (int32_t t = 0; t < ne; t++) {
    if (D == 3) {
      const V3 a = P(e[3 * t]), n = cross(sub(P(e[3 * t + 1]), a), sub(P(e[3 * t + 2]), a));
      const double l = norm(n);
      if (!(l > 0) || !std::isfinite(1.0 / l)) { wl_set_error(F + "triangle " + std::to_string(t) + " has zero area"); return WL_EINVAL; }
      nf[t] = mul(n, 1.0 / l);
    } else {
      const V3 d = sub(P(e[2 * t + 1]), P(e[2 * t]));
      const double l = norm(d);
      if (!(l > 0) || !std::isfinite(1.0 / l)) { wl_set_error(F + "segment " + std::to_string(t) + " has zero length"); return WL_EINVAL; }
      nf[t] = V3{d.y / l, -d.x / l, 0.0};                  // outward of a counter-clockwise polygon
    }
  }
  std::vector<int32_t> built;                               // 3-D: the triangle across edge k; 2-D: the segment into A (k = 0) / out of B (k = 1)
  if (!topo) built.assign((size_t)ne * D, -1);
  const std::vector<int32_t>& adj = topo ? *topo : built;
  if (topo) {
    WL_CHECK(topo->size() == (size_t)ne * D, "mesh tables: the kept adjacency does not belong to this connectivity");
  } else if (D == 3) {
    const std::string why = " is not shared by exactly two triangles in opposite directions: the surface is open, non-manifold or not oriented alike — "
                            "weld coincident vertices (unwelded triangle soup fails here) and give every triangle the same orientation";
    std::unordered_map<uint64_t, int32_t> dir;
    dir.reserve((size_t)ne * 3);
    for (int32_t t = 0; t < ne; t++)
      for (int k = 0; k < 3; k++) {
        const int32_t i = e[3 * t + k], j = e[3 * t + (k + 1) % 3];
        if (!dir.emplace(ekey(i, j), t).second) { wl_set_error(F + "edge (" + std::to_string(i) + ", " + std::to_string(j) + ")" + why); return WL_EINVAL; }
      }
    for (int32_t t = 0; t < ne; t++)
      for (int k = 0; k < 3; k++) {
        const int32_t i = e[3 * t + k], j = e[3 * t + (k + 1) % 3];
        const auto it = dir.find(ekey(j, i));
        if (it == dir.end()) { wl_set_error(F + "edge (" + std::to_string(i) + ", " + std::to_string(j) + ")" + why); return WL_EINVAL; }
        built[(size_t)3 * t + k] = it->second;
      }
  } else {
    std::vector<int32_t> in(nv, -1), og(nv, -1);
    std::vector<int32_t> nin(nv, 0), nog(nv, 0);
    for (int32_t t = 0; t < ne; t++) { og[e[2 * t]] = t; nog[e[2 * t]]++; in[e[2 * t + 1]] = t; nin[e[2 * t + 1]]++; }
    for (int32_t q = 0; q < nv; q++)
      if ((nin[q] || nog[q]) && !(nin[q] == 1 && nog[q] == 1)) {
        wl_set_error(F + "vertex " + std::to_string(q) + " has " + std::to_string(nin[q]) + " incoming and " + std::to_string(nog[q]) +
                     " outgoing segments, a closed polygon has exactly one incoming and one outgoing at every vertex (open or branching polyline; weld coincident vertices)");
        return WL_EINVAL;
      }
    for (int32_t t = 0; t < ne; t++) { built[(size_t)2 * t] = in[e[2 * t]]; built[(size_t)2 * t + 1] = og[e[2 * t + 1]]; }
  }
  double vol = 0;
  for (int32_t t = 0; t < ne; t++)
    vol += D == 3 ? dot(P(e[3 * t]), cross(P(e[3 * t + 1]), P(e[3 * t + 2]))) : P(e[2 * t]).x * P(e[2 * t + 1]).y - P(e[2 * t + 1]).x * P(e[2 * t]).y;
  if (!(vol > 0)) { wl_set_error(F + (D == 3 ? "the signed volume" : "the signed area") + " is not positive — the surface is oriented inward: reverse the index order of every element"); return WL_EINVAL; }

  out->D = D; out->ne = ne; out->scale = scale;
  out->elem.resize((size_t)ne * D * D); out->sph.resize((size_t)ne * 4); out->nrm.resize((size_t)ne * NR * D);
  std::vector<V3> vn;                                       // 3-D: Σ angle·n_face over the triangles around a vertex
  if (D == 3) {
    vn.assign(nv, V3{0, 0, 0});
    for (int32_t t = 0; t < ne; t++)
      for (int k = 0; k < 3; k++) {
        const V3 o = P(e[3 * t + k]), u = sub(P(e[3 * t + (k + 1) % 3]), o), w = sub(P(e[3 * t + (k + 2) % 3]), o);
        vn[e[3 * t + k]] = add(vn[e[3 * t + k]], mul(nf[t], std::atan2(norm(cross(u, w)), dot(u, w))));
      }
  }
  for (int32_t t = 0; t < ne; t++) {
    V3 p[3];
    for (int k = 0; k < D; k++) {
      p[k] = P(e[(size_t)D * t + k]);
      for (int d = 0; d < D; d++) out->elem[((size_t)t * D + k) * D + d] = v[(size_t)e[(size_t)D * t + k] * D + d];
    }
    V3 c; double r;
    bounding_sphere(p, D, &c, &r);
    float* s4 = &out->sph[(size_t)4 * t];
    s4[0] = (float)c.x; s4[1] = (float)c.y; s4[2] = (float)c.z;
    s4[3] = std::nextafter((float)(r * (1 + 1e-5) + 1e-6 * scale), INFINITY);      // outwards: the centre was rounded, the radius must still hold the element
    V3 rows[7];
    rows[0] = nf[t];
    if (D == 3)
      for (int k = 0; k < 3; k++) {
        rows[1 + k] = unit_or(add(nf[t], nf[adj[(size_t)3 * t + k]]), nf[t]);
        rows[4 + k] = unit_or(vn[e[3 * t + k]], nf[t]);
      }
    else
      for (int k = 0; k < 2; k++) rows[1 + k] = unit_or(add(nf[t], nf[adj[(size_t)2 * t + k]]), nf[t]);
    for (int q = 0; q < NR; q++) {
      float* n = &out->nrm[((size_t)t * NR + q) * D];
      n[0] = (float)rows[q].x; n[1] = (float)rows[q].y;
      if (D == 3) n[2] = (float)rows[q].z;
    }
  }
  if (!topo) out->adj = std::move(built);
  return 0;
}
int meshsdf_prepare(int D, const float* v, int32_t nv, const int32_t* e, int32_t ne, MeshTables* out, const char* who) {
  return prepare_tables(D, v, nv, e, ne, nullptr, out, who);
}
int meshsdf_prepare_geometry(int D, const float* v, int32_t nv, const int32_t* e, int32_t ne, const std::vector<int32_t>& adj, MeshTables* out, const char* who) {
  return prepare_tables(D, v, nv, e, ne, &adj, out, who);
}

int meshsdf_velocities(int D, const float* w, int32_t nv, const int32_t* e, int32_t ne, MeshTables* out, const char* who) {
  for (size_t q = 0; q < (size_t)nv * D; q++)
    if (!std::isfinite(w[q])) { wl_set_error(std::string(who) + ": the velocity of vertex " + std::to_string(q / D) + " is not finite"); return WL_EINVAL; }
  out->wtab.resize((size_t)ne * D * D);
  for (int32_t t = 0; t < ne; t++)
    for (int k = 0; k < D; k++)
      for (int d = 0; d < D; d++) out->wtab[((size_t)t * D + k) * D + d] = w[(size_t)e[(size_t)D * t + k] * D + d];
  return 0;
}

int meshsdf_run(const MeshTables& m, const int32_t* n, const float* c, float s, float band, unsigned flags, float* a_dev, float* a_host, float* w_dev, hipStream_t st) {
  const int D = m.D;
  const bool vel = w_dev != nullptr;
  WL_CHECK(!vel || m.wtab.size() == m.elem.size(), "mesh search: velocity samples asked for without a velocity table");
  using clk = std::chrono::steady_clock;
  const bool timed = g_ms_timed != 0;                      // wl_meshsdf_time: the phases are fenced with stream synchronisations and timed on the host
  auto t0 = clk::now();
  auto lap = [&](int q) -> int {
    if (!timed) return 0;
    WL_HIP(hipStreamSynchronize(st));
    const auto t1 = clk::now();
    g_ms_ms[q] = std::chrono::duration<double, std::milli>(t1 - t0).count(); t0 = t1;
    return 0;
  };
  MsArgs A{};
  A.ne = m.ne; A.s = s; A.brute = (flags & WL_MESH_BRUTE) ? 1 : 0; A.band = band;
  const int ext[3] = {4, D == 3 ? 4 : 16, D == 3 ? 4 : 1};
  double scale = std::fmax(m.scale, std::fabs((double)s));
  size_t count = 1;
  A.nbricks = 1;
  for (int d = 0; d < 3; d++) {
    A.n[d] = d < D ? n[d] : 1; A.c[d] = d < D ? c[d] : 0.f;
    A.nb[d] = (A.n[d] + ext[d] - 1) / ext[d];
    A.nbricks *= A.nb[d]; count *= (size_t)A.n[d];
    if (d < D) scale = std::fmax(scale, std::fmax(std::fabs((double)c[d] - s), std::fabs((double)c[d] + (double)s * A.n[d])));
  }
  // the brick's radius about its centre sample position, (ext − 1)/2 spacings per direction, rounded outwards; the slack: a relative 1e-4 of the bound (in
  // the kernel) plus this absolute part — Float32 rounding of positions and distances is below 1e-6 of the largest coordinate
  A.rb = (float)((D == 3 ? 2.5981 : 7.6486) * (double)s * (1 + 1e-5));
  A.slack = (float)(1e-4 * scale);
  const long nblocks = (A.nbricks + 3) / 4;
  WL_CHECK(nblocks <= 0x7fffffffL, "wl_sdf_lattice_from_mesh: too many bricks for one launch");
  // one scratch block: pairs | spheres | vertices | normals, each 16-byte aligned
  auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t b_pairs = up((size_t)A.nbricks * 8), b_sph = up(m.sph.size() * 4), b_elem = up(m.elem.size() * 4), b_nrm = up(m.nrm.size() * 4);
  const size_t b_wtab = vel ? up(m.wtab.size() * 4) : 0;
  char* base = (char*)wl_scratch(b_pairs + b_sph + b_elem + b_nrm + b_wtab);
  if (!base) return (int)hipErrorOutOfMemory;
  A.pairs = (unsigned long long*)base; A.sph = (const float4*)(base + b_pairs);
  A.elem = (const float*)(base + b_pairs + b_sph); A.nrm = (const float*)(base + b_pairs + b_sph + b_elem);
  A.a = a_dev;
  A.wtab = vel ? (const float*)(base + b_pairs + b_sph + b_elem + b_nrm) : nullptr; A.w = w_dev;
  WL_HIP(hipMemcpyAsync((void*)A.sph, m.sph.data(), m.sph.size() * 4, hipMemcpyHostToDevice, st));
  WL_HIP(hipMemcpyAsync((void*)A.elem, m.elem.data(), m.elem.size() * 4, hipMemcpyHostToDevice, st));
  WL_HIP(hipMemcpyAsync((void*)A.nrm, m.nrm.data(), m.nrm.size() * 4, hipMemcpyHostToDevice, st));
  if (vel) WL_HIP(hipMemcpyAsync((void*)A.wtab, m.wtab.data(), m.wtab.size() * 4, hipMemcpyHostToDevice, st));
  WL_TRY(lap(1));
#define MS_LAUNCH(D_, V_, B_) hipLaunchKernelGGL((k_meshsdf<D_, V_, B_>), dim3((unsigned)nblocks), dim3(256), 0, st, A)
  if (band > 0.f) {      // a lattice with a band: its own instantiations
    if (D == 3) { if (vel) MS_LAUNCH(3, true, true); else MS_LAUNCH(3, false, true); }
    else { if (vel) MS_LAUNCH(2, true, true); else MS_LAUNCH(2, false, true); }
  } else {
    if (D == 3) { if (vel) MS_LAUNCH(3, true, false); else MS_LAUNCH(3, false, false); }
    else { if (vel) MS_LAUNCH(2, true, false); else MS_LAUNCH(2, false, false); }
  }
#undef MS_LAUNCH
  WL_LAUNCH_CHECK();
  WL_TRY(lap(2));
  std::vector<unsigned long long> pairs((size_t)A.nbricks);
  WL_HIP(hipMemcpyAsync(a_host, a_dev, count * sizeof(float), hipMemcpyDeviceToHost, st));
  WL_HIP(hipMemcpyAsync(pairs.data(), A.pairs, pairs.size() * 8, hipMemcpyDeviceToHost, st));
  WL_HIP(hipStreamSynchronize(st));
  WL_TRY(lap(3));
  unsigned long long tested = 0, skipped = 0;
  for (unsigned long long q : pairs) { tested += q & ~MS_SKIPPED; skipped += q >> 63; }
  g_ms_searched = (unsigned long long)A.nbricks - skipped; g_ms_skipped = skipped;
  g_ms_tested = tested; g_ms_total = (unsigned long long)count * (unsigned long long)m.ne;
  return 0;
}
}  // namespace wl

extern "C" int wl_meshsdf_time(int on) { g_ms_timed = on ? 1 : 0; return 0; }
void wl::meshsdf_note_tables_ms(double ms) { g_ms_ms[0] = ms; }
extern "C" int wl_meshsdf_last_times(double* ms4) {
  WL_CHECK(ms4, "wl_meshsdf_last_times: null result");
  for (int q = 0; q < 4; q++) ms4[q] = g_ms_ms[q];
  return 0;
}
extern "C" int wl_meshsdf_last_bricks(uint64_t* searched, uint64_t* skipped) {
  WL_CHECK(searched && skipped, "wl_meshsdf_last_bricks: null result");
  *searched = g_ms_searched; *skipped = g_ms_skipped;
  return 0;
}
extern "C" int wl_meshsdf_last_pairs(uint64_t* tested, uint64_t* total) {
  WL_CHECK(tested && total, "wl_meshsdf_last_pairs: null result");
  *tested = g_ms_tested; *total = g_ms_total;
  return 0;
}
