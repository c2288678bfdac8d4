// What the Fourier diagnostics share: the column pass Z = F_H Y of the 2-D transform on the fp32 matrix pipe (spec_cols_kernel of
// tmg_spectrum.hip, xspec_cols_kernel of tmg_xspec.hip) and the temporal Fourier coefficient (tspec_finalize_kernel of tmg_tspec.hip,
// the fragments of tmg_spod.hip).  A header, compiled into each user with that file's own flags.  Written once here:
//   TMG_DFT_MAXN, tmg_dft_side_ok   the side of a 2-D transform: 16 <= N <= 512, a multiple of the 16-mode tile
//   tmg_fourier_coef                x - (s inv_t) g
//   the operand matrix, the MFMA lane maps and the column product, in the form given below
//
// Operand matrix of an N-point transform: T[n][m] = w[n] exp(-2 pi i ((n m) mod N) / N), planes (re, im) of [n][m] floats, built on the
// host in fp64 and rounded once.  The same layout is the row pass's B operand (k = n = x, column = m = q) and the column pass's A
// operand (k = n = y, row = m = p): in both a lane reads 16 consecutive floats of a row of T, and T (<= 2 MB) stays in L2.
// MFMA lane maps (16x16x4 f32): A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15], C/D column l & 15, rows 4 (l >> 4) + 0..3.
//
// The column product, as both column kernels write it (a member that equals the target gives the target's bits in the spectral
// skill because the two agree lane for lane and k for k; tests/test_xspec_cpu.py compares the text).  A block of 256 threads owns 16
// columns of one image; HP = 16 H:
//   stage   for (i = thread; i < HP; i += 256): lds[i] = re[(i >> 4) W + (i & 15)], lds[HP + i] = the same element of the im plane
//   lane    l16 = l & 15, lq = l >> 4;  br = lds + lq 16 + l16, bi = br + HP;  per row tile pt = wave, wave + 4, ..:
//           fr = ft + lq H + pt 16 + l16, fi = fr + H H
//   product zr = zi = 0; for k = 0, 4, .. < H (unrolled by four steps): a = (fr, fi)[k H], b = (br, bi)[k 16],
//           zr = mfma(a_r, b_r, zr), zi = mfma(a_r, b_i, zi), zr = mfma(-a_i, b_i, zr), zi = mfma(a_i, b_r, zi)
// Each kernel has its own epilogue under its own contraction setting (spec_cols_kernel: the default; xspec_cols_kernel: off).
// The staging and the product stay in the kernels.  They were tried as __forceinline__ functions of this header (staging into LDS;
// the row-tile product returning zr, zi by reference or as a struct): neither kernel compiled to the instructions it had, and with
// both behind functions xspec_cols_kernel took 0.259 ms against 0.238 ms (256 x 256, 64 images; 2.78 against 2.67 ms at 512 x 512) at
// two VGPRs fewer, spec_cols_kernel the same time.  With the staging alone behind a function the staging loop still came out
// differently, so both are kept where the compiler sees them as before, as tmg_symgram.h keeps its MFMA loop.
#pragma once
#include "tmg_common.h"

#define TMG_DFT_MAXN 512

static inline bool tmg_dft_side_ok(int64_t N) { return N >= 16 && N <= TMG_DFT_MAXN && (N & 15) == 0; }

// The Fourier coefficient of a windowed, centred series from its uncentred sum x = sum_n g_n x_n exp(..), the plain sum s = sum_n x_n,
// inv_t = fl(1 / Tn) and the window's own coefficient g: three roundings, xbar = fl(s inv_t), fl(xbar g), the subtraction.  All four
// users (tspec_finalize_kernel, both paths of spod_frag, the B fragment of spod_modes_kernel) are without contraction, so this is.
static __device__ __forceinline__ float tmg_fourier_coef(float x, float s, float inv_t, float g) {
#pragma clang fp contract(off)
    return x - (s * inv_t) * g;
}
