// Exchange buffer W of the pair smoother (wl_fused2_body.inc): what kernel A hands to kernel B behind a prolongation stage — r′ and ϵ_mid — as ONE
// float4 {r′.x, r′.y, ϵ_mid.x, ϵ_mid.y} per cell pair, in a layout of its own (both arrays have one writer, A, and one reader, B).
//   row    one 512-byte segment per core column of kernel A (ptile<2,2>: 60 cells = 30 pairs): 32 slots of 16 bytes, the pairs in slots 0..29,
//          slots 30 and 31 padding that nobody reads.  The 32 lanes of a wave row of A then write 512 contiguous, 512-byte aligned bytes: four whole
//          128-byte lines per store instruction, where the dense 8-byte stores on (4·nx)-byte rows leave lines partially written.
//   plane  ny rows, ghost rows included; nz planes, ghost planes included — zeroed once at allocation and never written, so kernel B finds there the
//          zeros it finds in the dense arrays.
// Plain C++ (no HIP): tests/test_abwide_cpu.py compiles this file on its own.
#pragma once
#if defined(__HIPCC__)
#define WL_ABW_HD __host__ __device__
#else
#define WL_ABW_HD
#endif
namespace wl {
constexpr int ABW_CX = 60;           // core cells per tile column of kernel A
constexpr unsigned ABW_SEG = 512;    // bytes per segment
constexpr unsigned ABW_ELT = 16;     // bytes per pair
WL_ABW_HD inline int abw_segments(int nx) { return (nx - 1 + ABW_CX - 1) / ABW_CX; }                    // = ptile<2,2>'s ntx
WL_ABW_HD inline unsigned abw_pitch(int nx) { return (unsigned)abw_segments(nx) * ABW_SEG; }           // bytes per row
// byte offset inside its row of the pair of cells (i0, i0+1), i0 even in [0, nx-2]
WL_ABW_HD inline unsigned abw_slot(int i0) { return (unsigned)(i0 / ABW_CX) * ABW_SEG + (unsigned)((i0 % ABW_CX) >> 1) * ABW_ELT; }
}  // namespace wl
