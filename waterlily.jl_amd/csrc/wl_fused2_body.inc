// Body of wl_fused2.hip, compiled once per tile height (WL_PT_Y rows of threads, namespace WL_PNS) — see wl_fused2.hip.


#define PT_X 32                      // threads along x (two cells each)
#define PT_Y WL_PT_Y
#define PT_N (PT_X * PT_Y)
#ifndef WL_P16_WAVES
#define WL_P16_WAVES 8
#endif
#define PT_WAVES (PT_N == 512 ? WL_P16_WAVES : 8)   // minimum waves per SIMD: 8 = two 1024-thread (four 512-thread) workgroups per CU, 64 VGPRs
// Occupancy target of kernels A / B.  With the fast steps the kernels hold the general step's and the fast steps' per-thread constants
// and want ≈90 VGPRs; capped at 64 they spill into the loop (B 0.72 -> 1.29 ms).  Both were measured insensitive to occupancy
// (profiles/r02_experiments.md), so the budget is 128 VGPRs: one 1024-thread (two 512-thread) workgroups per CU.
#ifndef WL_A_WAVES
#define WL_A_WAVES 4
#endif
#ifndef WL_B_WAVES
#define WL_B_WAVES 4
#endif
#define PL_W (PT_X + 2)              // LDS row: one guard entry on each side
#define PL_H ((PT_Y + 2) * PL_W)     // one parity array (guard rows above and below)
#define PL_SZ (2 * PL_H)             // a plane = even-x array followed by odd-x array

namespace WL_PNS {
namespace {

struct PTile {
  int i0, j;         // cell columns (i0, i0+1) × row j, 0-based with ghosts; i0 is even
  int lq;            // LDS index inside a parity array
  bool indom;        // the pair exists in the array
  bool in0, in1;     // cell 0 / cell 1 is an interior cell (may be updated)
  bool st0, st1;     // cell is stored by this workgroup (tile core ∧ interior)
  unsigned oc;       // i0 + j*sy
  int ks, ke;        // output planes [ks,ke)
  bool alive;
};

// HX (even) / HY: halo in cells.  Core of tile (tx,ty): cells [tx*CX, (tx+1)*CX) × rows [1+ty*CY, 1+(ty+1)*CY)
template <int HX, int HY>
__device__ __forceinline__ PTile ptile(const GridX& g, int zchunk) {
  PTile t;
  const int CX = 2 * PT_X - 2 * HX, CY = PT_Y - 2 * HY;
  const int ntx = (g.nx - 1 + CX - 1) / CX, nty = (g.ny - 2 + CY - 1) / CY;
  const int ntiles = ntx * nty;
  const unsigned h = blockIdx.x, q = h & 7u, s = h >> 3;
  const unsigned per = (unsigned)((ntiles + 7) >> 3);      // XCD q walks a contiguous range of tiles
  const int c = (int)(s / per);
  const int tl = (int)(q * per + (s - (unsigned)c * per));
  t.alive = tl < ntiles;
  const int tx = tl % ntx, ty = tl / ntx;
  // thread -> (lx, ly): the two 32-thread rows of a wave are PT_Y/2 rows apart, so all lanes of a wave have the same row parity
  // (the colour a thread updates in a sweep is then wave-uniform: the fast steps branch on it once instead of selecting per lane),
  // and the two halves of a wave fall onto disjoint LDS banks.
  const int lx = threadIdx.x & (PT_X - 1), ly = (int)(threadIdx.x >> 6) + (int)((threadIdx.x >> 5) & 1u) * (PT_Y / 2);
  t.i0 = tx * CX - HX + 2 * lx;
  t.j = 1 + ty * CY - HY + ly;
  t.lq = (ly + 1) * PL_W + lx + 1;
  t.indom = t.i0 >= 0 && t.i0 <= g.nx - 2 && t.j >= 0 && t.j < g.ny;
  const bool jin = t.j >= 1 && t.j <= g.ny - 2;
  t.in0 = t.indom && jin && t.i0 >= 2;
  t.in1 = t.indom && jin && t.i0 + 1 <= g.nx - 2;
  const bool corep = 2 * lx >= HX && 2 * lx < 2 * PT_X - HX && ly >= HY && ly < PT_Y - HY;
  t.st0 = corep && t.in0; t.st1 = corep && t.in1;
  t.oc = t.indom ? (unsigned)t.i0 + (unsigned)t.j * (unsigned)g.sy : 0u;
  t.ks = g.k0 + c * zchunk;
  t.ke = t.ks + zchunk < g.k1 ? t.ks + zchunk : g.k1;
  return t;
}
__host__ __device__ inline int ptile_count(int nx, int ny, int HX, int HY) {
  const int CX = 2 * PT_X - 2 * HX, CY = PT_Y - 2 * HY;
  return ((nx - 1 + CX - 1) / CX) * ((ny - 2 + CY - 1) / CY);
}
__device__ __forceinline__ float cf(int Ia, int Na, float c) { return (Ia <= 2 || Ia >= Na) ? 0.f : c; }
__device__ __forceinline__ float invd(float d) { return (d == 0.f) ? d : 1.0f / d; }
__device__ __forceinline__ float2 ld2(const float* __restrict__ p, unsigned o) { return *reinterpret_cast<const float2*>(p + o); }
__device__ __forceinline__ void st2(float* __restrict__ p, unsigned o, float2 v, bool s0, bool s1) {
  if (s0 && s1) *reinterpret_cast<float2*>(p + o) = v;
  else { if (s0) p[o] = v.x; if (s1) p[o + 1] = v.y; }
}
// plane K of the local array is an interior plane of the GLOBAL grid (single domain: k0 <= K < k1; on a z-slab also the
// neighbour's planes held as ghost planes, which the tile pipeline recomputes instead of waiting for them)
__device__ __forceinline__ bool pint(const GridX& g, int K) { const int Kg = g.gk + K; return K >= 0 && K < g.nz && Kg >= 1 && Kg <= g.gnz - 2; }
// quirk Q4 (half_rangek, src/Poisson.jl:123-132): an odd last dimension leaves its last plane unswept
__device__ __forceinline__ bool q4ok(const GridX& g, int Kg) { return !(Kg + 1 > 2 * (g.gnz / 2) - 1); }

// Per-thread constants of a constant-coefficient level
struct PCoef {
  float cxa, cxb, cxc;     // x-face coefficients: left of cell 0, between the cells, right of cell 1
  float ky, kyp;           // y-face coefficients below / above the row
  float dxy0, dxy1;        // (0 − (lx+lxp)) − (ly+lyp) of the two cells: set_diag!'s partial sum (src/Poisson.jl:49-55)
  float ide0, ide1;        // iD next to a z-wall (one z-face coefficient is 0), 0 for a ghost cell
  float idm0, idm1;        // iD with both z-faces open
};
__device__ __forceinline__ PCoef pcoef(const GridX& g, const PTile& t, const wl::ConstL& cl) {
  PCoef k;
  k.cxa = cf(t.i0 + 1, g.nx, cl.c[0]); k.cxb = cf(t.i0 + 2, g.nx, cl.c[0]); k.cxc = cf(t.i0 + 3, g.nx, cl.c[0]);
  k.ky = cf(t.j + 1, g.ny, cl.c[1]); k.kyp = cf(t.j + 2, g.ny, cl.c[1]);
  float s = 0.f; s -= (k.cxa + k.cxb); s -= (k.ky + k.kyp); k.dxy0 = s;
  s = 0.f; s -= (k.cxb + k.cxc); s -= (k.ky + k.kyp); k.dxy1 = s;
  const float ze = cl.c[2] + 0.f, zm = cl.c[2] + cl.c[2];     // lz+lzp: 0+c == c+0
  k.ide0 = t.in0 ? invd(k.dxy0 - ze) : 0.f; k.ide1 = t.in1 ? invd(k.dxy1 - ze) : 0.f;
  k.idm0 = t.in0 ? invd(k.dxy0 - zm) : 0.f; k.idm1 = t.in1 ? invd(k.dxy1 - zm) : 0.f;
  return k;
}

// One colour sweep on a pair: the active cell (act1 ? cell 1 : cell 0) gets gauss(I,…) (src/Poisson.jl:116-122).
//   S: LDS plane holding the x-y neighbours; ep: the plane's pair (updated); em/en: the planes below/above; rp: r; d: iD.
__device__ __forceinline__ void pair_sweep(const float* __restrict__ S, int off_oth, int off_y, bool act1, bool gate, float lxo, const PCoef& k,
                                           float lzl, float lzu, const float2& rp, const float2& d, const float2& em, const float2& en, float2& ep) {
  const float oth = S[off_oth];                          // the x-neighbour owned by the adjacent thread
  const float ym = S[off_y - PL_W], yp = S[off_y + PL_W];
  const float partv = act1 ? ep.x : ep.y;                // the x-neighbour inside the pair
  float s = act1 ? rp.y : rp.x;
  s -= (oth * lxo + partv * k.cxb);                      // ϵ[I−δx]·L[I,1] + ϵ[I+δx]·L[I+δx,1] (either order, same bits)
  s -= (ym * k.ky + yp * k.kyp);
  s -= ((act1 ? em.y : em.x) * lzl + (act1 ? en.y : en.x) * lzu);
  const float v = s * (act1 ? d.y : d.x);
  if (gate) { if (act1) ep.y = v; else ep.x = v; }
}

// The hardware's vector-memory counter retires loads and stores in issue order, and a store of this pipeline is conditional (tile
// core only), so the compiler can only wait for "everything" (vmcnt(0)) when the prefetched plane is first used.  If that use comes
// right after the step's stores — as it does when the stores end one step and the register rotation starts the next — every step
// waits for a full store round trip.  The kernels therefore force the use (an empty asm that reads the prefetched registers) just
// BEFORE their stores: the wait then covers loads issued a whole step earlier and stores issued a whole step earlier.
#define WL_SETTLE2(a, b) asm volatile("" ::"v"((a).x), "v"((a).y), "v"((b).x), "v"((b).y) : "memory")
#define WL_SETTLE3(a, b, c) asm volatile("" ::"v"((a).x), "v"((a).y), "v"((b).x), "v"((b).y), "v"((c).x), "v"((c).y) : "memory")

// byte-offset accessors: a uniform base pointer + a 32-bit per-lane offset (fields hold < 2^30 elements) selects the
// scalar-base addressing mode of global loads/stores: no 64-bit address arithmetic per access
__device__ __forceinline__ float2 ldb(const float* __restrict__ p, unsigned bo) { return *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(p) + bo); }
__device__ __forceinline__ void stb(float* __restrict__ p, unsigned bo, float2 v) { *reinterpret_cast<float2*>(reinterpret_cast<char*>(p) + bo) = v; }
// Buffer-addressed accesses for the fast steps.  A lane (or a whole step) that must not load/store is given an offset beyond the
// buffer's num_records: the hardware's range check drops the store / returns 0 for the load.  The instruction itself is issued
// unconditionally, so every fast step issues the SAME number of vector-memory operations and the compiler can place counted waits
// (`s_waitcnt vmcnt(N)`: gfx950 retires loads and stores in issue order) instead of draining everything with vmcnt(0) — a conditional
// store (exec-masked behind an `s_cbranch_execz`) makes the count unknowable and forces the drain.
typedef unsigned wl_v2u __attribute__((ext_vector_type(2)));
#define WL_OOB_LANE 0x40000000u      // per-lane "no access" offset   (fields hold < 2^30 BYTES·4 … the sums below never wrap into range:
#define WL_OOB_STEP 0x80000000u      // uniform "not in this step"     valid < 2^30·… ; LANE|STEP = 0xC0000000; + plane offset < 2^32)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mkbuf(const float* p, unsigned bytes) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, (int)bytes, 0x00020000); }
__device__ __forceinline__ float2 bld2(__amdgpu_buffer_rsrc_t b, unsigned voff, unsigned soff) {
  const wl_v2u t = __builtin_amdgcn_raw_buffer_load_b64(b, (int)voff, (int)soff, 0);
  return make_float2(__uint_as_float(t.x), __uint_as_float(t.y));
}
__device__ __forceinline__ void bst2(__amdgpu_buffer_rsrc_t b, unsigned voff, unsigned soff, float2 v) {
  wl_v2u t; t.x = __float_as_uint(v.x); t.y = __float_as_uint(v.y);
  __builtin_amdgcn_raw_buffer_store_b64(t, b, (int)voff, (int)soff, 0);
}
// 16-byte forms for the exchange buffer W (wl_abwide.hpp).  W may exceed the 2^30 bytes the flags above assume, so a workgroup's descriptor covers only the
// planes of its own z-chunk: base = the chunk's first plane, num_records = those planes (gsrb_pair_wide_bytes bounds them by 2^30: a flagged offset is then
// >= num_records whatever in-range plane offset is added, and a valid lane offset + plane offset stays below num_records)
typedef unsigned wl_v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t mkbufw(const float* p, size_t byte0, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(reinterpret_cast<const char*>(p)) + byte0, 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ float4 bld4(__amdgpu_buffer_rsrc_t b, unsigned voff, unsigned soff) {
  const wl_v4u t = __builtin_amdgcn_raw_buffer_load_b128(b, (int)voff, (int)soff, 0);
  return make_float4(__uint_as_float(t.x), __uint_as_float(t.y), __uint_as_float(t.z), __uint_as_float(t.w));
}
__device__ __forceinline__ void bst4(__amdgpu_buffer_rsrc_t b, unsigned voff, unsigned soff, float4 v) {
  wl_v4u t; t.x = __float_as_uint(v.x); t.y = __float_as_uint(v.y); t.z = __float_as_uint(v.z); t.w = __float_as_uint(v.w);
  __builtin_amdgcn_raw_buffer_store_b128(t, b, (int)voff, (int)soff, 0);
}
__device__ __forceinline__ float4 ldw(const float* __restrict__ W, size_t bo) { return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(W) + bo); }
__device__ __forceinline__ void stw(float* __restrict__ W, size_t bo, float4 v) { *reinterpret_cast<float4*>(reinterpret_cast<char*>(W) + bo) = v; }
// kernel A's wide store: 1 — every lane of a stored tile row stores, the two halo lanes (and lanes beyond the array) zeros into padding slots, so a wave row is one
// whole 512-byte burst; 0 — only the lanes that own a pair store.  Measured per instance (profiles/abwide_experiments.md §4): the burst wins on the 32-row
// instance (512² planes: A 479 -> 418 µs), the plain form on the 16-row one (258² planes: 67 -> 58 µs — the last segment of a 258-cell row is 70 % padding)
#ifndef WL_ABW_PAD
#define WL_ABW_PAD (PT_Y == 32)
#endif
static_assert(2 * PT_X - 4 == wl::ABW_CX, "a segment of W is a core column of kernel A");
// timing ablations (experiments; wrong results): -DWL_ABL_NOSTORE drops every store of the fast steps, -DWL_ABL_NOLOAD every load,
// -DWL_ABL_NOBAR removes the fast steps' barrier
#ifdef WL_ABL_NOSTORE
#define WL_STBYTES(b) 0u
#else
#define WL_STBYTES(b) (b)
#endif
#ifdef WL_ABL_NOLOAD
#define WL_LDBYTES(b) 0u
#else
#define WL_LDBYTES(b) (b)
#endif
#ifdef WL_ABL_NOBAR
#define WL_FAST_SYNC() do { } while (0)
#else
#define WL_FAST_SYNC() __syncthreads()
#endif
#ifdef WL_STAMP   // DIAGNOSTIC build (tools/build_variant.sh stamp "-fno-slp-vectorize -DWL_STAMP" wl_fused2.hip; tools/stamp_A.py): where a fast step of kernel A
                  // spends its cycles, per wave (s_memtime).  Never in the product build.
__device__ unsigned long long g_wl_stamp[8];
__device__ __forceinline__ unsigned long long wl_stamp() { unsigned long long t; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory"); return t; }
#define WL_ST(var) const unsigned long long var = wl_stamp()
#else
#define WL_ST(var)
#endif
struct CTrue { static constexpr bool value = true; };
struct CFalse { static constexpr bool value = false; };

#define WL_SETTLE4(a, b, c, d) asm volatile("" ::"v"((a).x), "v"((a).y), "v"((b).x), "v"((b).y), "v"((c).x), "v"((c).y), "v"((d).x), "v"((d).y) : "memory")
struct __attribute__((packed, aligned(4))) F2U { float x, y; };   // two adjacent floats at a 4-byte aligned address: one 8-byte load
__device__ __forceinline__ float2 ld2u(const float* __restrict__ p, unsigned o) { const F2U v = *reinterpret_cast<const F2U*>(p + o); return make_float2(v.x, v.y); }
// The V-cycle's `x += ω·x_c↓` (increment! after prolongate!, src/MultiLevelPoisson.jl:99-100) deferred from kernel A to kernel B: B applies it
// to the x it loads, before its own `x += ω·ϵ` — the same two additions in the same order, but x makes one round trip instead of two.
struct XPro { const float* xc; int on; float w; int cx, cy, cz; unsigned csy, csz; int cgk; unsigned cbytes; };

struct ProArgs2 { const float* xc; float* x; float* rnew; GridX gc; int cx, cy, cz; float w;
                  int xk0, xk1;      // planes on which x is updated (z-slabs: the launch may cover ghost planes for r' and ϵ_mid, x only the owned ones)
                  int zoff; };       // PRO == 2: local coarse plane of the fine local plane K = ((K+1)>>1) + zoff  (z-slabs: g.gk/2 − gc.gk, g.gk even; else 0)
__device__ __forceinline__ int dwn(int i, int c) { return c ? (i + 1) / 2 : i; }   // down(I,c), 0-based  src/MultiLevelPoisson.jl:7

// ------------------------------------------------------------------------------------------------------------------
// kernel A:  [PRO: r' = r − ω·A(x_c↓), x += ω·x_c↓  (Vcycle!'s prolongate!+increment!, src/MultiLevelPoisson.jl:99-100)]
//            ϵ = r·iD ; colour sweep 1 ; colour sweep 2  →  ϵ_mid
// ------------------------------------------------------------------------------------------------------------------
// WIDE (only with PRO, and only when x is left to kernel B): `emid` is the level's exchange buffer W.  r′ and ϵ_mid of plane K−2 leave together, as one 16-byte
// store at step K (r′ of that plane is still in r2); rnew, x and the dense emid are not touched.
template <int PRO, int WIDE = 0>
__global__ void __launch_bounds__(PT_N, WL_A_WAVES) k_gsrb2_A(GridX g, float* __restrict__ emid, const float* __restrict__ r, int zchunk, ProArgs2 pa, wl::ConstL cl) {
  __shared__ float sA[2][PL_SZ];   // ϵ⁰ of the newest plane
  __shared__ float sB[2][PL_SZ];   // plane K-1 after sweep 1
  const PTile t = ptile<2, 2>(g, zchunk);
  if (!t.alive) return;
  for (int q = threadIdx.x; q < PL_SZ; q += PT_N) { sA[0][q] = 0.f; sA[1][q] = 0.f; sB[0][q] = 0.f; sB[1][q] = 0.f; }
  const PCoef k = pcoef(g, t, cl);
  const float c2 = cl.c[2];
  const int jpar = (t.j + g.gk) & 1;
  const int oth0 = PL_H + t.lq - 1, oth1 = t.lq + 1;       // cell 0 active: odd cell of the left thread; cell 1: even cell of the right thread
  float2 e0 = {0.f, 0.f}, e1 = e0, e2 = e0, e3 = e0, r0 = e0, r1 = e0, r2 = e0, n_r0;
  const int Kbeg = t.ks - 2, Kend = t.ke + 1;
  // coarse columns under the pair and its x-neighbours (PRO)
  unsigned q0 = 0, q1 = 0, q2 = 0, q3 = 0, cj0 = 0, cjm = 0, cjp = 0;
  if (PRO == 1 && t.indom && t.j >= 1 && t.j <= g.ny - 2) {
    q0 = (unsigned)dwn(t.i0 > 0 ? t.i0 - 1 : 0, pa.cx); q1 = (unsigned)dwn(t.i0, pa.cx); q2 = (unsigned)dwn(t.i0 + 1, pa.cx);
    q3 = (unsigned)dwn(t.i0 + 2 <= g.nx - 1 ? t.i0 + 2 : g.nx - 1, pa.cx);
    cj0 = (unsigned)dwn(t.j, pa.cy) * (unsigned)pa.gc.sy; cjm = (unsigned)dwn(t.j - 1, pa.cy) * (unsigned)pa.gc.sy; cjp = (unsigned)dwn(t.j + 1, pa.cy) * (unsigned)pa.gc.sy;
  }
  // PRO == 2: every direction is coarsened (the usual case).  The pair (i0,i0+1) and its x-neighbours lie over the two coarse
  // columns qa, qa+1; of the rows j±1 (planes K±1) one lies over the cell's own coarse row (plane), the other over the
  // next one — by the parity of j (K).  Six coarse values per step, kept in registers: Cc (own plane, own row), Co (own
  // plane, other row), Cz (other plane, own row); when K advances either Cz or — after Cc and Cz trade places — Co is
  // replaced by two values fetched one step ahead.  2 loads per step instead of 12.
  const bool jodd = (t.j & 1) != 0;
  unsigned rc = 0, ro = 0;                 // qa + coarse row offset (own / other row)
  const int nzc = pa.gc.nz;
  float2 Cc = {0.f, 0.f}, Co = Cc, Cz = Cc, n_c = Cc, n_x0 = Cc;
  auto cpl = [&](int p) { p += pa.zoff; return (unsigned)(p < 0 ? 0 : (p > nzc - 1 ? nzc - 1 : p)) * (unsigned)pa.gc.sz; };   // p: coarse plane in the fine level's local frame
  if (PRO == 2) {
    if (t.indom) {
      const unsigned qa = (unsigned)(t.i0 >> 1), cr = (unsigned)((t.j + 1) >> 1);
      rc = qa + cr * (unsigned)pa.gc.sy;
      ro = qa + (jodd ? cr - 1u : cr + 1u) * (unsigned)pa.gc.sy;
    }
    const int m = (Kbeg + 1) >> 1, zo = (Kbeg & 1) ? m - 1 : m + 1;
    Cc = make_float2(pa.xc[rc + cpl(m)], pa.xc[rc + cpl(m) + 1]);
    Co = make_float2(pa.xc[ro + cpl(m)], pa.xc[ro + cpl(m) + 1]);
    Cz = make_float2(pa.xc[rc + cpl(zo)], pa.xc[rc + cpl(zo) + 1]);
  }
  auto fetch = [&](int K) {
    const bool pl0 = t.indom && pint(g, K);                     // r of ghost planes/cells is 0
    const unsigned o = t.oc + (unsigned)K * (unsigned)g.sz;
    n_r0 = pl0 ? ld2(r, o) : make_float2(0.f, 0.f);
    if (PRO && !WIDE) n_x0 = ((t.st0 || t.st1) && K >= t.ks && K < t.ke && K >= pa.xk0 && K < pa.xk1) ? ld2(pa.x, o) : make_float2(0.f, 0.f);
    if (PRO == 2) {   // coarse values that become current at step K: plane m(K-1)+1; own row if K is even, other row if odd
      const unsigned a = ((K & 1) ? ro : rc) + cpl((K >> 1) + 1);
      n_c = make_float2(pa.xc[a], pa.xc[a + 1]);
    }
  };
  fetch(Kbeg);
  n_c = Cz;    // (the state for Kbeg was loaded directly; make the first transition below a no-op)
  if (PRO == 2) WL_SETTLE3(n_r0, n_x0, n_c); else if (PRO) WL_SETTLE2(n_r0, n_x0); else WL_SETTLE2(n_r0, n_r0);   // (no load pending at the loop entry either: the loop top then needs no wait at all)
  // ---- fast steps (see kernel B): planes K-2..K+2 away from the z-walls and inside the local array, no clamping of the coarse plane
  const float zs2 = c2 + c2;
  const float pd0 = t.in0 ? k.dxy0 - zs2 : 0.f, pd1 = t.in1 ? k.dxy1 - zs2 : 0.f;
  const unsigned sz4 = (unsigned)g.sz * 4u, ob0 = t.oc * 4u;
  const bool stp = t.st0 || t.st1;
  int Kf0 = Kbeg + 1, Kf1 = Kend;                                  // fast steps [Kf0, Kf1)
  if (Kf0 < 4 - g.gk) Kf0 = 4 - g.gk;
  if (Kf0 < 2) Kf0 = 2;
  if (Kf1 > g.gnz - 2 - g.gk) Kf1 = g.gnz - 2 - g.gk;
  if (Kf1 > g.nz - 1) Kf1 = g.nz - 1;
  if (PRO == 2 && Kf1 > 2 * (nzc - pa.zoff) - 4) Kf1 = 2 * (nzc - pa.zoff) - 4;   // ((K+1)>>1)+1+zoff <= nzc-1
  if (PRO == 2 && Kf0 < -2 * pa.zoff) Kf0 = -2 * pa.zoff;                          // ((K+1)>>1)+1+zoff >= 0 with room to spare
  Kf0 += Kf0 & 1;
  if (PRO == 1 || (g.gk & 1) || Kf1 < Kf0) Kf1 = Kf0;
  Kf1 -= (Kf1 - Kf0) & 1;
  const unsigned fbytes = (unsigned)(g.cs * 4);
  const __amdgpu_buffer_rsrc_t b_r = mkbuf(r, WL_LDBYTES(fbytes)), b_x = mkbuf(pa.x, WL_LDBYTES(fbytes)), b_xs = mkbuf(pa.x, WL_STBYTES(fbytes)), b_rn = mkbuf(pa.rnew, WL_STBYTES(fbytes)), b_em = mkbuf(emid, WL_STBYTES(fbytes));
  const unsigned vst = stp ? ob0 : WL_OOB_LANE;                    // store offset of the lane (tile core ∧ interior), else out of range
  // WIDE: bytes per plane of W, the pair's offset inside a plane, the chunk's descriptor (planes [ks,ke): the ones this workgroup stores) and the lane's store offset
  const unsigned wpl = WIDE ? (unsigned)g.ny * wl::abw_pitch(g.nx) : 0u;
  const unsigned wo = (WIDE && t.indom) ? (unsigned)t.j * wl::abw_pitch(g.nx) + wl::abw_slot(t.i0) : 0u;
  const __amdgpu_buffer_rsrc_t b_w = mkbufw(emid, WIDE ? (size_t)t.ks * wpl : 0, WIDE ? WL_STBYTES((unsigned)(t.ke - t.ks) * wpl) : 0u);
  unsigned wst = stp ? wo : WL_OOB_LANE;
  if (WIDE && WL_ABW_PAD) {   // every lane of a core row that is an interior row: lane lx -> slot (lx − 1) mod 32 of the tile's segment (the pair's own slot for the core lanes)
    const int lx = threadIdx.x & (PT_X - 1), ly = (int)(threadIdx.x >> 6) + (int)((threadIdx.x >> 5) & 1u) * (PT_Y / 2);
    const bool row = ly >= 2 && ly < PT_Y - 2 && t.j >= 1 && t.j <= g.ny - 2;
    const unsigned seg = (unsigned)((t.i0 + 2 - 2 * lx) / wl::ABW_CX);
    wst = row ? (unsigned)t.j * wl::abw_pitch(g.nx) + seg * wl::ABW_SEG + (unsigned)((lx + PT_X - 1) & (PT_X - 1)) * wl::ABW_ELT : WL_OOB_LANE;
  }
#ifdef WL_STAMP
  unsigned long long st_pre = 0, st_bar = 0, st_swp = 0, st_sto = 0, st_n = 0;
#endif
  auto fast = [&](auto jodd_c) {
    constexpr bool JODD = decltype(jodd_c)::value;
    auto step = [&](auto kodd_c, const int K) {
      constexpr bool KODD = decltype(kodd_c)::value;
      constexpr bool ACT1 = JODD != KODD;
      constexpr int pb = KODD ? 0 : 1, cb = KODD ? 1 : 0;
      WL_ST(T0);
      e3 = e2; e2 = e1; e1 = e0; r2 = r1; r1 = r0; r0 = n_r0;
      const float2 x0 = n_x0;
      if (PRO == 2) {
        if (KODD) { const float2 tmp = Cc; Cc = Cz; Cz = tmp; Co = n_c; }
        else Cz = n_c;
      }
      const unsigned pk = (unsigned)K * sz4;                        // byte offset of plane K
      n_r0 = bld2(b_r, ob0, pk + sz4);                              // (lanes outside the array read the plane's corner ghost pair)
      if (PRO && !WIDE) n_x0 = bld2(b_x, vst | ((K + 1 >= t.ks && K + 1 < t.ke && K + 1 >= pa.xk0 && K + 1 < pa.xk1) ? 0u : WL_OOB_STEP), pk + sz4);
      if (PRO == 2) {
        const unsigned a = (KODD ? rc : ro) + (unsigned)(((K + 1) >> 1) + 1 + pa.zoff) * (unsigned)pa.gc.sz;   // K+1 odd: the other coarse row
        n_c = make_float2(pa.xc[a], pa.xc[a + 1]);
      }
      float2 xs = {0.f, 0.f};
      if (PRO) {   // increment!(fine;ω) with ϵ = x_c[down(I)], z-face coefficients c[2]
        const float va = Cc.x, v0 = Cc.x, v1 = Cc.y, vb = Cc.y;
        const float ym0 = JODD ? Co.x : Cc.x, yp0 = JODD ? Cc.x : Co.x, ym1 = JODD ? Co.y : Cc.y, yp1 = JODD ? Cc.y : Co.y;
        const float zm0 = KODD ? Cz.x : Cc.x, zp0 = KODD ? Cc.x : Cz.x, zm1 = KODD ? Cz.y : Cc.y, zp1 = KODD ? Cc.y : Cz.y;
        float s = v0 * pd0;
        s += (va * k.cxa + v1 * k.cxb);
        s += (ym0 * k.ky + yp0 * k.kyp);
        s += (zm0 * c2 + zp0 * c2);
        r0.x = t.in0 ? r0.x - pa.w * s : r0.x;
        s = v1 * pd1;
        s += (v0 * k.cxb + vb * k.cxc);
        s += (ym1 * k.ky + yp1 * k.kyp);
        s += (zm1 * c2 + zp1 * c2);
        r0.y = t.in1 ? r0.y - pa.w * s : r0.y;
        // (a pair on an x-wall holds one ghost cell: it is written back unchanged, so every store is a whole pair)
        if (!WIDE) xs = make_float2(t.st0 ? x0.x + pa.w * v0 : x0.x, t.st1 ? x0.y + pa.w * v1 : x0.y);
      }
      e0.x = r0.x * k.idm0; e0.y = r0.y * k.idm1;                   // ϵ = r·iD
#ifdef WL_STAMP
      asm volatile("" :: "v"(e0.x), "v"(e0.y));      // the prolongation stage (and the wait for this step's operands) ends here
#endif
      WL_ST(T1);
      WL_FAST_SYNC();
      WL_ST(T2);
      auto sweep = [&](const float* __restrict__ S, const float2& rp, const float2& em, const float2& en, float2& ep) {
        const float oth = S[ACT1 ? oth1 : oth0];
        const float ym = S[(ACT1 ? t.lq + PL_H : t.lq) - PL_W], yp = S[(ACT1 ? t.lq + PL_H : t.lq) + PL_W];
        const float partv = ACT1 ? ep.x : ep.y;
        float s = ACT1 ? rp.y : rp.x;
        s -= (oth * (ACT1 ? k.cxc : k.cxa) + partv * k.cxb);
        s -= (ym * k.ky + yp * k.kyp);
        s -= ((ACT1 ? em.y : em.x) * c2 + (ACT1 ? en.y : en.x) * c2);
        const float v = s * (ACT1 ? k.idm1 : k.idm0);
        if (ACT1) ep.y = t.in1 ? v : ep.y; else ep.x = t.in0 ? v : ep.x;
      };
      if (K - 1 >= t.ks - 1) sweep(sA[pb], r1, e2, e0, e1);        // sweep 1 on plane K-1
      if (K - 2 >= t.ks) sweep(sB[pb], r2, e3, e1, e2);            // sweep 2 on plane K-2
      sA[cb][t.lq] = e0.x; sA[cb][t.lq + PL_H] = e0.y;
      sB[cb][t.lq] = e1.x; sB[cb][t.lq + PL_H] = e1.y;
      WL_ST(T3);
      // all stores of the step, issued unconditionally (see mkbuf): the next step's first use of n_r0/n_x0/n_c waits with a counted vmcnt
      if (WIDE) {
        const bool own2 = (K - 2) >= t.ks && (K - 2) < t.ke;
        const float4 v = (!WL_ABW_PAD || stp) ? make_float4(r2.x, r2.y, e2.x, e2.y) : make_float4(0.f, 0.f, 0.f, 0.f);
        bst4(b_w, wst | (own2 ? 0u : WL_OOB_STEP), own2 ? (unsigned)(K - 2 - t.ks) * wpl : 0u, v);
      } else {
      if (PRO) {
        const bool own = K >= t.ks && K < t.ke;
        bst2(b_rn, vst | (own ? 0u : WL_OOB_STEP), pk, r0);
        bst2(b_xs, vst | ((own && K >= pa.xk0 && K < pa.xk1) ? 0u : WL_OOB_STEP), pk, xs);
      }
      bst2(b_em, vst | (((K - 2) >= t.ks && (K - 2) < t.ke) ? 0u : WL_OOB_STEP), pk - 2u * sz4, e2);
      }
#ifdef WL_STAMP
      { WL_ST(T4); st_pre += T1 - T0; st_bar += T2 - T1; st_swp += T3 - T2; st_sto += T4 - T3; st_n++; }
#endif
    };
    for (int K = Kf0; K < Kf1; K += 2) { step(CFalse{}, K); step(CTrue{}, K + 1); }
#ifdef WL_STAMP
    if (PRO == 2 && (threadIdx.x & 63) == 0) {
      atomicAdd(&g_wl_stamp[0], st_pre); atomicAdd(&g_wl_stamp[1], st_bar); atomicAdd(&g_wl_stamp[2], st_swp); atomicAdd(&g_wl_stamp[3], st_sto); atomicAdd(&g_wl_stamp[4], st_n);
    }
#endif
  };
  const bool jodd_u = __builtin_amdgcn_readfirstlane(t.j & 1) != 0;
  for (int K = Kbeg; K <= Kend; K++) {
    if (K == Kf0 && Kf1 > Kf0) {
      if (jodd_u) fast(CTrue{}); else fast(CFalse{});
      K = Kf1;
      if (K > Kend) break;
    }
    e3 = e2; e2 = e1; e1 = e0; r2 = r1; r1 = r0; r0 = n_r0;
    const float2 x0 = n_x0;
    if (PRO == 2 && K > Kbeg) {
      if (K & 1) { const float2 tmp = Cc; Cc = Cz; Cz = tmp; Co = n_c; }
      else Cz = n_c;
    }
    if (K < Kend) fetch(K + 1);                                     // a whole step ahead of its use
    const unsigned o0 = t.oc + (unsigned)K * (unsigned)g.sz;
    const bool plK = pint(g, K);
    float2 xs = {0.f, 0.f};                                         // PRO: the new x of plane K (stored at the end of the step)
    const float lz0 = cf(g.gk + K + 1, g.gnz, c2), lzp0 = cf(g.gk + K + 2, g.gnz, c2);          // z-faces below / above plane K
    const float lz1 = cf(g.gk + K, g.gnz, c2), lz2 = cf(g.gk + K - 1, g.gnz, c2);
    if (PRO && plK) {   // increment!(fine;ω) with ϵ = x_c[down(I)]          src/Poisson.jl:100-104, mult :70-76
      float va, v0, v1, vb, ym0, yp0, ym1, yp1, zm0, zp0, zm1, zp1;
      if (PRO == 2) {
        const bool kodd = (K & 1) != 0;
        va = Cc.x; v0 = Cc.x; v1 = Cc.y; vb = Cc.y;
        ym0 = jodd ? Co.x : Cc.x; yp0 = jodd ? Cc.x : Co.x; ym1 = jodd ? Co.y : Cc.y; yp1 = jodd ? Cc.y : Co.y;
        zm0 = kodd ? Cz.x : Cc.x; zp0 = kodd ? Cc.x : Cz.x; zm1 = kodd ? Cz.y : Cc.y; zp1 = kodd ? Cc.y : Cz.y;
      } else {
        const int Kg = g.gk + K;
        const unsigned ck0 = (unsigned)(dwn(Kg, pa.cz) - pa.gc.gk) * (unsigned)pa.gc.sz, ckm = (unsigned)(dwn(Kg - 1, pa.cz) - pa.gc.gk) * (unsigned)pa.gc.sz,
                       ckp = (unsigned)(dwn(Kg + 1, pa.cz) - pa.gc.gk) * (unsigned)pa.gc.sz;
        const float* __restrict__ xc = pa.xc;
        va = xc[q0 + cj0 + ck0]; v0 = xc[q1 + cj0 + ck0]; v1 = xc[q2 + cj0 + ck0]; vb = xc[q3 + cj0 + ck0];
        ym0 = xc[q1 + cjm + ck0]; yp0 = xc[q1 + cjp + ck0]; ym1 = xc[q2 + cjm + ck0]; yp1 = xc[q2 + cjp + ck0];
        zm0 = xc[q1 + cj0 + ckm]; zp0 = xc[q1 + cj0 + ckp]; zm1 = xc[q2 + cj0 + ckm]; zp1 = xc[q2 + cj0 + ckp];
      }
      const float zs = lz0 + lzp0;
      float s = v0 * (t.in0 ? k.dxy0 - zs : 0.f);
      s += (va * k.cxa + v1 * k.cxb);
      s += (ym0 * k.ky + yp0 * k.kyp);
      s += (zm0 * lz0 + zp0 * lzp0);
      if (t.in0) r0.x = r0.x - pa.w * s;
      s = v1 * (t.in1 ? k.dxy1 - zs : 0.f);
      s += (v0 * k.cxb + vb * k.cxc);
      s += (ym1 * k.ky + yp1 * k.kyp);
      s += (zm1 * lz0 + zp1 * lzp0);
      if (t.in1) r0.y = r0.y - pa.w * s;
      if (!WIDE) xs = make_float2(x0.x + pa.w * v0, x0.y + pa.w * v1);
    }
    {   // ϵ = r·iD   :142   (ghost cells and planes: iD = 0)
      const bool edge = (lz0 == 0.f) || (lzp0 == 0.f);
      const float d0x = plK ? (edge ? k.ide0 : k.idm0) : 0.f, d0y = plK ? (edge ? k.ide1 : k.idm1) : 0.f;
      e0.x = r0.x * d0x; e0.y = r0.y * d0y;
    }
    __syncthreads();                                                // LDS of the previous step is complete
    const int pb = (K - 1) & 1, cb = K & 1;
    const bool act1 = ((jpar ^ K) & 1) != 0;
    const bool gate = act1 ? t.in1 : t.in0;
    const int off_oth = act1 ? oth1 : oth0, off_y = act1 ? t.lq + PL_H : t.lq;
    const float lxo = act1 ? k.cxc : k.cxa;
    // ---- sweep 1 on plane K-1
    if (pint(g, K - 1) && (K - 1) >= t.ks - 1 && q4ok(g, g.gk + K - 1)) {
      const bool edge = (lz1 == 0.f) || (lz0 == 0.f);
      const float2 d = make_float2(edge ? k.ide0 : k.idm0, edge ? k.ide1 : k.idm1);
      pair_sweep(sA[pb], off_oth, off_y, act1, gate, lxo, k, lz1, lz0, r1, d, e2, e0, e1);
    }
    // ---- sweep 2 on plane K-2
    if (pint(g, K - 2) && (K - 2) >= t.ks && q4ok(g, g.gk + K - 2)) {
      const bool edge = (lz2 == 0.f) || (lz1 == 0.f);
      const float2 d = make_float2(edge ? k.ide0 : k.idm0, edge ? k.ide1 : k.idm1);
      pair_sweep(sB[pb], off_oth, off_y, act1, gate, lxo, k, lz2, lz1, r2, d, e3, e1, e2);
    }
    sA[cb][t.lq] = e0.x; sA[cb][t.lq + PL_H] = e0.y;
    sB[cb][t.lq] = e1.x; sB[cb][t.lq + PL_H] = e1.y;
    // ---- all stores of the step, behind the wait for the prefetched plane (see WL_SETTLE)
    if (PRO == 2) WL_SETTLE3(n_r0, n_x0, n_c); else if (PRO) WL_SETTLE2(n_r0, n_x0); else WL_SETTLE2(n_r0, n_r0);
    if (WIDE) {   // (the planes [ks,ke) are interior planes: what the dense form stores of r′ at step K−2 and of ϵ_mid at step K, the pair written whole)
      if (stp && (K - 2) >= t.ks && (K - 2) < t.ke) stw(emid, (size_t)(K - 2) * wpl + wo, make_float4(r2.x, r2.y, e2.x, e2.y));
    } else
    if (t.st0 || t.st1) {
      if (PRO && plK && K >= t.ks && K < t.ke) {
        st2(pa.rnew, o0, r0, t.st0, t.st1);
        if (K >= pa.xk0 && K < pa.xk1) st2(pa.x, o0, xs, t.st0, t.st1);
      }
      if ((K - 2) >= t.ks && (K - 2) < t.ke) st2(emid, o0 - 2u * (unsigned)g.sz, e2, t.st0, t.st1);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// kernel B:  colour sweep 3 ; colour sweep 4 ; increment!(ω)  [NORMS: L₁, L∞ of r' per workgroup; EPS: store the final ϵ]
// OUT (wl::BOut): which of increment!'s two results are stored.  B_BOTH: r' and x.  B_XONLY: no store to rout is issued at all (r' lives in registers for the
// norms; the launch leaves ϵ_mid and r untouched, so B_RONLY can produce rout later).  B_RONLY: sweeps 3 and 4 and r' as ever, rout stored; x and x_c are
// neither loaded nor stored, no norms.  The statements that produce r' and x are the same in every mode.
// ------------------------------------------------------------------------------------------------------------------
// WIDE: `emid` is the level's exchange buffer W and `r` is not read: one 16-byte load per step brings ϵ_mid of plane K+1 and r′ of plane K+1 — r′ one plane
// earlier than the dense form loads it, so it is carried one more step (r0).
template <int NORMS, int EPS, int OUT = wl::B_BOTH, int WIDE = 0>
__global__ void __launch_bounds__(PT_N, WL_B_WAVES) k_gsrb2_B(GridX g, float* __restrict__ eout, float* __restrict__ rout, float* __restrict__ x, const float* __restrict__ emid,
                                                     const float* __restrict__ r, float w, int zchunk, double* __restrict__ part, float* __restrict__ pmax, wl::ConstL cl, XPro xp) {
  __shared__ float sA[2][PL_SZ];   // ϵ_mid of the newest plane
  __shared__ float sB[2][PL_SZ];   // plane K-1 after sweep 3
  __shared__ float sC[2][PL_SZ];   // plane K-2 after sweep 4 = final ϵ
  const PTile t = ptile<4, 3>(g, zchunk);
  if (!t.alive) { if (NORMS && threadIdx.x == 0) { part[blockIdx.x] = 0.0; pmax[blockIdx.x] = 0.f; } return; }
  for (int q = threadIdx.x; q < PL_SZ; q += PT_N) { sA[0][q] = 0.f; sA[1][q] = 0.f; sB[0][q] = 0.f; sB[1][q] = 0.f; sC[0][q] = 0.f; sC[1][q] = 0.f; }
  const PCoef k = pcoef(g, t, cl);
  const float c2 = cl.c[2];
  const int jpar = (t.j + g.gk) & 1;
  const int oth0 = PL_H + t.lq - 1, oth1 = t.lq + 1;
  float2 e0 = {0.f, 0.f}, e1 = e0, e2 = e0, e3 = e0, e4 = e0, r1 = e0, r2 = e0, r3 = e0, n_e0, n_r1, n_x3 = e0, n_v3 = e0;
  float2 r0 = e0;                  // WIDE: r′ of plane K (n_r1 then holds r′ of the plane n_e0 is of)
  const unsigned wpl = WIDE ? (unsigned)g.ny * wl::abw_pitch(g.nx) : 0u;                                            // bytes per plane of W
  const unsigned wo = (WIDE && t.indom) ? (unsigned)t.j * wl::abw_pitch(g.nx) + wl::abw_slot(t.i0) : 0u;            // the pair inside a plane (lanes outside the array: the corner ghost pair, zeros)
  double nsum = 0.0; float nmax = 0.f;
  const int Kbeg = t.ks - 3, Kend = t.ke + 2;
  const bool stp = t.st0 || t.st1;
  const unsigned qxc = (xp.on && t.indom) ? (unsigned)dwn(t.i0, xp.cx) + (unsigned)dwn(t.j, xp.cy) * xp.csy : 0u;   // the pair's coarse parents: xc[qxc], xc[qxc+1] (+ plane)
  auto fetch = [&](int K) {
    const unsigned o0 = t.oc + (unsigned)K * (unsigned)g.sz;
    if (WIDE) {   // (ghost planes of W hold zeros: the r′ of a plane that is not interior)
      const float4 v = (t.indom && K >= 0 && K <= g.nz - 1) ? ldw(emid, (size_t)K * wpl + wo) : make_float4(0.f, 0.f, 0.f, 0.f);
      n_r1 = make_float2(v.x, v.y); n_e0 = make_float2(v.z, v.w);
    } else {
    n_e0 = (t.indom && K >= 0 && K <= g.nz - 1) ? ld2(emid, o0) : make_float2(0.f, 0.f);
    n_r1 = (t.indom && pint(g, K - 1)) ? ld2(r, o0 - (unsigned)g.sz) : make_float2(0.f, 0.f);
    }
    if (OUT != wl::B_RONLY) {
    n_x3 = (stp && (K - 3) >= t.ks && (K - 3) < t.ke) ? ld2(x, o0 - 3u * (unsigned)g.sz) : make_float2(0.f, 0.f);
    if (xp.on && stp && (K - 3) >= t.ks && (K - 3) < t.ke) n_v3 = ld2u(xp.xc, qxc + (unsigned)(dwn(g.gk + K - 3, xp.cz) - xp.cgk) * xp.csz);
    }
  };
  fetch(Kbeg);
  if (OUT != wl::B_RONLY) WL_SETTLE4(n_e0, n_r1, n_x3, n_v3); else WL_SETTLE2(n_e0, n_r1);   // (no load pending at the loop entry: the loop top then needs no wait at all)
  // ---- fast steps -------------------------------------------------------------------------------------------------------------
  // A step whose planes K-3..K+1 are all away from the z-walls (every z-face coefficient = c[2], iD = the "both faces open" value)
  // and inside the local array needs none of the general step's plane predicates, and — the colour a wave updates being uniform
  // (ptile's row map) and alternating with K — none of its per-lane colour selects: the steps below are the general step with
  // those values folded (same operations on the same operands ⇒ same bits), two per iteration, for both row parities.  What remains
  // per step are the chunk-range conditions (uniform scalar branches) and the per-lane interior / tile-core masks.
  const float zs2 = c2 + c2;
  const float dI0 = k.dxy0 - zs2, dI1 = k.dxy1 - zs2;
  const unsigned sz4 = (unsigned)g.sz * 4u, ob0 = t.oc * 4u;
  int Kf0 = Kbeg, Kf1 = Kend;                                      // fast steps [Kf0, Kf1)
  if (Kf0 < 5 - g.gk) Kf0 = 5 - g.gk;
  if (Kf1 > g.gnz - 1 - g.gk) Kf1 = g.gnz - 1 - g.gk;
  if (Kf1 > g.nz - 1) Kf1 = g.nz - 1;
  Kf0 += Kf0 & 1;
  if ((g.gk & 1) || Kf1 < Kf0) Kf1 = Kf0;
  Kf1 -= (Kf1 - Kf0) & 1;
  const unsigned fbytes = (unsigned)(g.cs * 4);
  const __amdgpu_buffer_rsrc_t b_em = mkbuf(emid, WL_LDBYTES(fbytes)), b_r = mkbuf(r, WL_LDBYTES(fbytes)), b_x = mkbuf(x, WL_LDBYTES(fbytes)), b_xs = mkbuf(x, WL_STBYTES(fbytes)), b_ro = mkbuf(rout, WL_STBYTES(fbytes)), b_xc = mkbuf(xp.xc, xp.cbytes);
  const unsigned vst = stp ? ob0 : WL_OOB_LANE;                    // store offset of the lane (tile core ∧ interior), else out of range
  const unsigned vxc = stp ? qxc * 4u : WL_OOB_LANE;               // the pair's coarse parents
  // WIDE: the chunk's descriptor over the planes this workgroup reads, [max(Kbeg,0), min(Kend,nz−1)]; every lane's load is in range
  const int wp0 = Kbeg > 0 ? Kbeg : 0, wp1 = Kend < g.nz - 1 ? Kend : g.nz - 1;
  const __amdgpu_buffer_rsrc_t b_w = mkbufw(emid, WIDE ? (size_t)wp0 * wpl : 0, WIDE ? WL_LDBYTES((unsigned)(wp1 - wp0 + 1) * wpl) : 0u);
  auto fast = [&](auto jodd_c) {
    constexpr bool JODD = decltype(jodd_c)::value;
    auto step = [&](auto kodd_c, const int K) {
      constexpr bool KODD = decltype(kodd_c)::value;
      constexpr bool ACT1 = JODD != KODD;                           // the cell of the pair that this colour sweep updates
      constexpr int pb = KODD ? 0 : 1, cb = KODD ? 1 : 0;
      e4 = e3; e3 = e2; e2 = e1; e1 = e0; r3 = r2; r2 = r1;
      e0 = n_e0;
      if (WIDE) { r1 = r0; r0 = n_r1; } else r1 = n_r1;
      const float2 x3 = xp.on ? make_float2(n_x3.x + xp.w * n_v3.x, n_x3.y + xp.w * n_v3.y) : n_x3;
      const unsigned pk = (unsigned)K * sz4;                        // byte offset of plane K
      if (WIDE) {
        const float4 v = bld4(b_w, wo, (unsigned)(K + 1 - wp0) * wpl);
        n_r1 = make_float2(v.x, v.y); n_e0 = make_float2(v.z, v.w);
      } else {
      n_e0 = bld2(b_em, ob0, pk + sz4);                             // (lanes outside the array read the plane's corner ghost pair)
      n_r1 = bld2(b_r, ob0, pk);
      }
      if (OUT != wl::B_RONLY) {
        const unsigned mo = ((K - 2) >= t.ks && (K - 2) < t.ke) ? 0u : WL_OOB_STEP;
        n_x3 = bld2(b_x, vst | mo, pk - 2u * sz4);
        if (xp.on) n_v3 = bld2(b_xc, vxc | mo, (unsigned)(dwn(g.gk + K - 2, xp.cz) - xp.cgk) * (xp.csz * 4u));
      }
      WL_FAST_SYNC();
      auto sweep = [&](const float* __restrict__ S, const float2& rp, const float2& em, const float2& en, float2& ep) {
        const float oth = S[ACT1 ? oth1 : oth0];
        const float ym = S[(ACT1 ? t.lq + PL_H : t.lq) - PL_W], yp = S[(ACT1 ? t.lq + PL_H : t.lq) + PL_W];
        const float partv = ACT1 ? ep.x : ep.y;
        float s = ACT1 ? rp.y : rp.x;
        s -= (oth * (ACT1 ? k.cxc : k.cxa) + partv * k.cxb);
        s -= (ym * k.ky + yp * k.kyp);
        s -= ((ACT1 ? em.y : em.x) * c2 + (ACT1 ? en.y : en.x) * c2);
        const float v = s * (ACT1 ? k.idm1 : k.idm0);
        if (ACT1) ep.y = t.in1 ? v : ep.y; else ep.x = t.in0 ? v : ep.x;
      };
      if (K - 1 >= t.ks - 2) sweep(sA[pb], r1, e2, e0, e1);        // sweep 3 on plane K-1
      if (K - 2 >= t.ks - 1) sweep(sB[pb], r2, e3, e1, e2);        // sweep 4 on plane K-2
      const bool inc = (K - 3) >= t.ks && (K - 3) < t.ke;           // increment! on plane K-3
      float2 rn = {0.f, 0.f}, xn = {0.f, 0.f};
      if (inc) {
        const float* __restrict__ S = sC[pb];
        float s = e3.x * dI0;
        s += (S[oth0] * k.cxa + e3.y * k.cxb);
        s += (S[t.lq - PL_W] * k.ky + S[t.lq + PL_W] * k.kyp);
        s += (e4.x * c2 + e2.x * c2);
        const float rn0 = r3.x - w * s;
        s = e3.y * dI1;
        s += (e3.x * k.cxb + S[oth1] * k.cxc);
        s += (S[PL_H + t.lq - PL_W] * k.ky + S[PL_H + t.lq + PL_W] * k.kyp);
        s += (e4.y * c2 + e2.y * c2);
        const float rn1 = r3.y - w * s;
        // the pairs on the x-walls hold one ghost cell: it is written back unchanged, so every store is a whole pair
        rn = make_float2(t.st0 ? rn0 : r3.x, t.st1 ? rn1 : r3.y);
        xn = make_float2(t.st0 ? x3.x + w * e3.x : x3.x, t.st1 ? x3.y + w * e3.y : x3.y);
        if (NORMS) {
          const float a0 = t.st0 ? fabsf(rn0) : 0.f, a1 = t.st1 ? fabsf(rn1) : 0.f;
          nsum += (double)a0; nsum += (double)a1; nmax = fmaxf(nmax, fmaxf(a0, a1));
        }
      }
      sA[cb][t.lq] = e0.x; sA[cb][t.lq + PL_H] = e0.y;
      sB[cb][t.lq] = e1.x; sB[cb][t.lq + PL_H] = e1.y;
      sC[cb][t.lq] = e2.x; sC[cb][t.lq + PL_H] = e2.y;
      {   // all stores of the step, issued unconditionally (see mkbuf): counted waits instead of a drain per step
        const unsigned mo = inc ? 0u : WL_OOB_STEP;
        if (OUT != wl::B_XONLY) bst2(b_ro, vst | mo, pk - 3u * sz4, rn);
        if (OUT != wl::B_RONLY) bst2(b_xs, vst | mo, pk - 3u * sz4, xn);
        if (EPS && inc && stp) st2(eout, t.oc + (unsigned)(K - 3) * (unsigned)g.sz, e3, t.st0, t.st1);   // (test-only variant: its conditional store costs it the counted waits)
      }
    };
    for (int K = Kf0; K < Kf1; K += 2) { step(CFalse{}, K); step(CTrue{}, K + 1); }
  };
  const bool jodd_u = __builtin_amdgcn_readfirstlane(t.j & 1) != 0;
  for (int K = Kbeg; K <= Kend; K++) {
    if (K == Kf0 && Kf1 > Kf0) {
      if (jodd_u) fast(CTrue{}); else fast(CFalse{});
      K = Kf1;
      if (K > Kend) break;
    }
    e4 = e3; e3 = e2; e2 = e1; e1 = e0; r3 = r2; r2 = r1;
    e0 = n_e0;
    if (WIDE) { r1 = r0; r0 = n_r1; } else r1 = n_r1;
    const float2 x3 = xp.on ? make_float2(n_x3.x + xp.w * n_v3.x, n_x3.y + xp.w * n_v3.y) : n_x3;
    if (K < Kend) fetch(K + 1);
    const float lz0 = cf(g.gk + K + 1, g.gnz, c2), lz1 = cf(g.gk + K, g.gnz, c2), lz2 = cf(g.gk + K - 1, g.gnz, c2), lz3 = cf(g.gk + K - 2, g.gnz, c2);
    __syncthreads();
    const int pb = (K - 1) & 1, cb = K & 1;
    const bool act1 = ((jpar ^ K) & 1) != 0;
    const bool gate = act1 ? t.in1 : t.in0;
    const int off_oth = act1 ? oth1 : oth0, off_y = act1 ? t.lq + PL_H : t.lq;
    const float lxo = act1 ? k.cxc : k.cxa;
    // ---- sweep 3 on plane K-1
    if (pint(g, K - 1) && (K - 1) >= t.ks - 2 && q4ok(g, g.gk + K - 1)) {
      const bool edge = (lz1 == 0.f) || (lz0 == 0.f);
      const float2 d = make_float2(edge ? k.ide0 : k.idm0, edge ? k.ide1 : k.idm1);
      pair_sweep(sA[pb], off_oth, off_y, act1, gate, lxo, k, lz1, lz0, r1, d, e2, e0, e1);
    }
    // ---- sweep 4 on plane K-2
    if (pint(g, K - 2) && (K - 2) >= t.ks - 1 && q4ok(g, g.gk + K - 2)) {
      const bool edge = (lz2 == 0.f) || (lz1 == 0.f);
      const float2 d = make_float2(edge ? k.ide0 : k.idm0, edge ? k.ide1 : k.idm1);
      pair_sweep(sB[pb], off_oth, off_y, act1, gate, lxo, k, lz2, lz1, r2, d, e3, e1, e2);
    }
    // ---- increment! on plane K-3: r' = r − ω·Aϵ ; x += ω·ϵ          src/Poisson.jl:100-104, mult :70-76
    const bool inc = stp && (K - 3) >= t.ks && (K - 3) < t.ke;
    float2 rn = {0.f, 0.f}, xn = {0.f, 0.f};
    if (inc) {
      const float* __restrict__ S = sC[pb];
      const float zs = lz3 + lz2;
      float s = e3.x * (k.dxy0 - zs);
      s += (S[oth0] * k.cxa + e3.y * k.cxb);
      s += (S[t.lq - PL_W] * k.ky + S[t.lq + PL_W] * k.kyp);
      s += (e4.x * lz3 + e2.x * lz2);
      const float rn0 = r3.x - w * s;
      s = e3.y * (k.dxy1 - zs);
      s += (e3.x * k.cxb + S[oth1] * k.cxc);
      s += (S[PL_H + t.lq - PL_W] * k.ky + S[PL_H + t.lq + PL_W] * k.kyp);
      s += (e4.y * lz3 + e2.y * lz2);
      const float rn1 = r3.y - w * s;
      rn = make_float2(rn0, rn1);
      xn = make_float2(x3.x + w * e3.x, x3.y + w * e3.y);
      if (NORMS) {
        const float a0 = t.st0 ? fabsf(rn0) : 0.f, a1 = t.st1 ? fabsf(rn1) : 0.f;
        nsum += (double)a0; nsum += (double)a1; nmax = fmaxf(nmax, fmaxf(a0, a1));
      }
    }
    sA[cb][t.lq] = e0.x; sA[cb][t.lq + PL_H] = e0.y;
    sB[cb][t.lq] = e1.x; sB[cb][t.lq + PL_H] = e1.y;
    sC[cb][t.lq] = e2.x; sC[cb][t.lq + PL_H] = e2.y;
    // ---- all stores of the step, behind the wait for the prefetched plane (see WL_SETTLE)
    if (OUT != wl::B_RONLY) WL_SETTLE4(n_e0, n_r1, n_x3, n_v3); else WL_SETTLE2(n_e0, n_r1);
    if (inc) {
      const unsigned o3 = t.oc + (unsigned)(K - 3) * (unsigned)g.sz;
      if (OUT != wl::B_XONLY) st2(rout, o3, rn, t.st0, t.st1);
      if (OUT != wl::B_RONLY) st2(x, o3, xn, t.st0, t.st1);
      if (EPS) st2(eout, o3, e3, t.st0, t.st1);
    }
  }
  if (NORMS) {   // 16 waves -> one partial per workgroup
    __shared__ double shs[PT_N / 64]; __shared__ float shm[PT_N / 64];
    nsum = wave_sum(nsum); nmax = wave_max(nmax);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shs[threadIdx.x >> 6] = nsum; shm[threadIdx.x >> 6] = nmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
      double a = 0.0; float mx = 0.f;
      for (int q = 0; q < PT_N / 64; q++) { a += shs[q]; mx = fmaxf(mx, shm[q]); }
      part[blockIdx.x] = a; pmax[blockIdx.x] = mx;
    }
  }
}

int zchunk2(const GridX& g, int HX, int HY) {
  const int nt = ptile_count(g.nx, g.ny, HX, HY);
  const int np = g.k1 - g.k0;
  static const int target = wl_exp_int("WL_PAIR_WGS", 0);
  static const int zmin_env = wl_exp_int("WL_ZC_MIN", 0);
  static const int ch_a = wl_exp_int("WL_PAIR_CH_A", 0), ch_b = wl_exp_int("WL_PAIR_CH_B", 0);   // experiments: number of z-chunks of kernel A / B
  if ((HY == 3 ? ch_b : ch_a) > 0) { const int c = HY == 3 ? ch_b : ch_a; int zc = (np + c - 1) / c; if (zc < 4) zc = 4; if (zc > np) zc = np; return zc; }
  if (target) {   // experiments: fixed workgroup target
    int chunks = target >= 0 ? (target + nt - 1) / nt : (-target) / nt; if (chunks < 1) chunks = 1;
    int zc = (np + chunks - 1) / chunks; const int zmin = zmin_env ? zmin_env : 4; if (zc < zmin) zc = zmin; if (zc > np) zc = np;
    return zc;
  }
  // Equal workgroups, dealt to the XCDs tile range by tile range (ptile), run in rounds of 32 CUs × (1024 / PT_N) resident workgroups per XCD:
  // choose the chunk length that minimises   rounds × (planes per chunk + pipeline warm-up),
  // i.e. trade the warm-up recomputation of short chunks against the idle tail of a partly filled last round; few rounds pay a
  // balance penalty (wall tiles and the first / last chunk are slower).  Measured at 512³ (tools/chscan.sh): kernel A 1.05 -> 0.97 ms per
  // step against the former fixed target of 3072 workgroups (13 rounds, the last one almost empty).  Grids that cannot fill one round
  // are bound by the per-plane latency of the march: shortest chunks (>= 4 planes).
  const int warm = (HY == 3 ? 5 : 3) + 3;
  const long per = (nt + 7) >> 3, SX = 32L * (1024 / PT_N);
  double best = -1.0; int best_zc = np;
  for (int chunks = 1; chunks <= np; chunks++) {
    const int zc = (np + chunks - 1) / chunks;
    if (zc < (zmin_env ? zmin_env : 4)) break;
    const int nch = (np + zc - 1) / zc;
    const long W = per * nch;
    const long rounds = (W + SX - 1) / SX;
    double cost = (double)rounds * (zc + warm) * (1.0 + 0.3 / (double)rounds);
    if (W < SX) cost = (zc + warm) * 1.3;          // a partly filled chip still pays the full per-plane latency (and unbalanced CUs)
    if (best < 0 || cost < best) { best = cost; best_zc = zc; }
  }
  return best_zc;
}
}  // namespace

int gsrb_pair_A(float* emid, const float* r, const GridX& g, const wl::ConstL& cl, hipStream_t s) {
  const int zc = zchunk2(g, 2, 2);
  const int nt = ptile_count(g.nx, g.ny, 2, 2), per = (nt + 7) >> 3, nch = (g.k1 - g.k0 + zc - 1) / zc;
  ProArgs2 pa{};
  hipLaunchKernelGGL((k_gsrb2_A<0>), dim3((unsigned)(8 * per * nch)), dim3(PT_N), 0, s, g, emid, r, zc, pa, cl);
  WL_LAUNCH_CHECK(); return 0;
}
int gsrb_pair_A_pro(float* emid, float* rnew, float* x, const float* r, const float* xc, const GridX& g, const GridX& gc, float w, const wl::ConstL& cl, hipStream_t s,
                    int xk0 = -(1 << 30), int xk1 = 1 << 30, float* wide = nullptr) {
  const int zc = zchunk2(g, 2, 2);
  const int nt = ptile_count(g.nx, g.ny, 2, 2), per = (nt + 7) >> 3, nch = (g.k1 - g.k0 + zc - 1) / zc;
  ProArgs2 pa{xc, x, rnew, gc, gc.nx < g.nx, gc.ny < g.ny, gc.gnz < g.gnz, w, xk0, xk1, 0};
  // every direction coarsened by two: the register-window form (PRO == 2).  On a z-slab the fine local plane K is the global plane g.gk+K; with an
  // even g.gk its parity is K's and its coarse parent is the local coarse plane ((K+1)>>1) + g.gk/2 − gc.gk (gc may be a slab or a replicated level).
  const bool fullc = pa.cx && pa.cy && pa.cz && (g.gk & 1) == 0 && 2 * (gc.nx - 2) == g.nx - 2 && 2 * (gc.ny - 2) == g.ny - 2 && 2 * (gc.gnz - 2) == g.gnz - 2;
  if (fullc) pa.zoff = g.gk / 2 - gc.gk;
  if (wide) {   // r′ and ϵ_mid to the exchange buffer; x is kernel B's
    if (xk0 < xk1) { wl_set_error("gsrb_pair_A_pro: the wide exchange needs the x increment deferred to kernel B"); return WL_EINVAL; }
    if (fullc && g_pro_fast) hipLaunchKernelGGL((k_gsrb2_A<2, 1>), dim3((unsigned)(8 * per * nch)), dim3(PT_N), 0, s, g, wide, r, zc, pa, cl);
    else hipLaunchKernelGGL((k_gsrb2_A<1, 1>), dim3((unsigned)(8 * per * nch)), dim3(PT_N), 0, s, g, wide, r, zc, pa, cl);
    WL_LAUNCH_CHECK(); return 0;
  }
  if (fullc && g_pro_fast) hipLaunchKernelGGL((k_gsrb2_A<2>), dim3((unsigned)(8 * per * nch)), dim3(PT_N), 0, s, g, emid, r, zc, pa, cl);
  else hipLaunchKernelGGL((k_gsrb2_A<1>), dim3((unsigned)(8 * per * nch)), dim3(PT_N), 0, s, g, emid, r, zc, pa, cl);
  WL_LAUNCH_CHECK(); return 0;
}
int gsrb_pair_B(float* eps, float* rout, float* x, const float* emid, const float* r, const GridX& g, float w,
                const RedWs* ws, int slot_d, int slot_f, const wl::ConstL& cl, hipStream_t s, const wl::XDefer* xd, int out, const float* wide) {
  XPro xp{};
  if (out == wl::B_RONLY) { ws = nullptr; xd = nullptr; eps = nullptr; }   // the recompute of a skipped rout: no x, no norms, no ϵ
  if (xd) xp = XPro{xd->xc, 1, xd->w, xd->gc.nx < g.nx, xd->gc.ny < g.ny, xd->gc.gnz < g.gnz, (unsigned)xd->gc.sy, (unsigned)xd->gc.sz, xd->gc.gk, (unsigned)(xd->gc.cs * 4)};
  const int zc = zchunk2(g, 4, 3);
  const int nt = ptile_count(g.nx, g.ny, 4, 3), per = (nt + 7) >> 3, nch = (g.k1 - g.k0 + zc - 1) / zc;
  const unsigned nb = (unsigned)(8 * per * nch);
  const bool norms = ws && nb <= WL_MAXPART;
  double* pa = norms ? ws->pa : nullptr; float* pm = norms ? ws->pm : nullptr;
#define WL_GB(NF, EF) hipLaunchKernelGGL((k_gsrb2_B<NF, EF>), dim3(nb), dim3(PT_N), 0, s, g, eps, rout, x, emid, r, w, zc, pa, pm, cl, xp)
#define WL_GBO(NF, OF) hipLaunchKernelGGL((k_gsrb2_B<NF, 0, OF>), dim3(nb), dim3(PT_N), 0, s, g, eps, rout, x, emid, r, w, zc, pa, pm, cl, xp)
#define WL_GBW(NF, OF) hipLaunchKernelGGL((k_gsrb2_B<NF, 0, OF, 1>), dim3(nb), dim3(PT_N), 0, s, g, eps, rout, x, wide, (const float*)nullptr, w, zc, pa, pm, cl, xp)
  if (wide) {   // ϵ_mid and r′ from the exchange buffer kernel A's wide form filled
    if (eps || (ws && !norms)) { wl_set_error("gsrb_pair_B: the wide exchange stores no ϵ and needs its norms from the kernel"); return WL_EINVAL; }
    if (out == wl::B_XONLY) { if (norms) WL_GBW(1, wl::B_XONLY); else WL_GBW(0, wl::B_XONLY); }
    else if (out == wl::B_RONLY) WL_GBW(0, wl::B_RONLY);
    else { if (norms) WL_GBW(1, wl::B_BOTH); else WL_GBW(0, wl::B_BOTH); }
  } else
  if (out == wl::B_XONLY) {
    // (the fallback norms below read the stored array: the caller asks gsrb_pair_B_kernel_norms first)
    if (eps || (ws && !norms)) { wl_set_error("gsrb_pair_B: the x-only form stores no ϵ and needs its norms from the kernel"); return WL_EINVAL; }
    if (norms) WL_GBO(1, wl::B_XONLY); else WL_GBO(0, wl::B_XONLY);
  } else if (out == wl::B_RONLY) WL_GBO(0, wl::B_RONLY);
  else
  if (norms) { if (eps) WL_GB(1, 1); else WL_GB(1, 0); } else { if (eps) WL_GB(0, 1); else WL_GB(0, 0); }
#undef WL_GBW
#undef WL_GBO
#undef WL_GB
  if (norms) WL_TRY(wl::finalize_sum_max(*ws, (int)nb, slot_d, slot_f, s));
  else if (ws) WL_TRY(wl::norms_dev(rout, g, *ws, slot_d, slot_f, s));
  WL_LAUNCH_CHECK(); return 0;
}
// the longest z-chunk of kernels A and B on this grid (the planes a workgroup's descriptor over W spans are at most this + 7)
int wide_chunk_planes(const GridX& g) { const int a = zchunk2(g, 2, 2), b = zchunk2(g, 4, 3); return a > b ? a : b; }
// the launch of gsrb_pair_B for this grid takes its norms from the kernel's registers (not from the stored rout)
bool gsrb_pair_B_kernel_norms(const GridX& g) {
  const int zc = zchunk2(g, 4, 3);
  const int nt = ptile_count(g.nx, g.ny, 4, 3), per = (nt + 7) >> 3, nch = (g.k1 - g.k0 + zc - 1) / zc;
  return (unsigned)(8 * per * nch) <= WL_MAXPART;
}
}  // namespace WL_PNS

#undef PT_X
#undef PT_Y
#undef PT_N
#undef PT_WAVES
#undef PL_W
#undef PL_H
#undef PL_SZ
