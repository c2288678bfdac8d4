/* Spectral POD of the ensemble members (tmg_spod.hip): per case and frequency bin the Hermitian member-by-member cross-spectral density
 * matrix, a Gram product over the pixels of the planar Fourier coefficients that tmg_tspec_block accumulates, and the synthesis of the
 * modes from host-built weights, both on the fp32 matrix pipe; partials in a workspace, no float atomics: bitwise reproducible.
 * A header of its own: tmglow_hip.h (which defines tmg_stream_t) does not include it. */
#ifndef TMGLOW_HIP_SPOD_H
#define TMGLOW_HIP_SPOD_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The operand of both kernels is tmg_tspec_block's accumulator acc [2 NF + 1][R][B][C][HW] over R = S + 1 rows (the S members, then the
 * target) with cst [3][NF] = (Re G_k, Im G_k, c_k / Tn^2).  For row m, bin k, channel c and pixel p, exactly as tspec_finalize_kernel
 * (no contraction): xbar = acc[2 NF] * fl(1 / Tn), Re X_m = acc[k] - xbar G_re, Im X_m = acc[NF + k] - xbar G_im.
 *
 * tmg_ens_spod_plan launches nothing: the launch plan of tmg_ens_spod_csd and tmg_ens_spod_modes for dims = {S, B, Cg, HW, NB, addr}
 * (Cg selected channels, NB selected bins, addr the address of acc or 0), which the launch bodies themselves call.
 * plan (9 host integers) = {P, L, NP, ws, SL, NT, part, vec, MB}:
 *   NT  row macro-tiles of 64 rows over the 2 R rows Z = [Re X_0 .. Re X_{R-1}; Im X_0 .. Im X_{R-1}]; NP = NT (NT + 1) / 2 macro-tile
 *       pairs I <= J, pair (I, J) at index I NT - I (I - 1) / 2 + (J - I); only the upper triangle is computed
 *   P   pixel slices, slice s = pixels [s SL, min(HW, (s + 1) SL)) of every selected channel, SL a multiple of 256; chosen so that
 *       B NB NP P blocks fill the device while ws stays under 2^24 floats (P = 1 may exceed that)
 *   L   = Cg SL: the fmaf terms of one partial (four waves' chains of Cg SL / 4 end to end, then 3 additions in wave order): L P >= Cg HW
 *   part  floats of one partial: 4096 (a 64 x 64 macro-tile pair), or 256 when 2 R <= 16 (one 16-row tile: the small instance)
 *   ws  floats of workspace: B NB NP part (P + 1) for P > 1 (the partials, then their sums in slice order), B NB NP part for P = 1
 *   vec 1: the rows are read with 16-byte loads (HW a multiple of 4 and addr a multiple of 16), 0: with scalar loads
 *   MB  blocks of 256 pixels of the modes kernel (its grid is MB x Cg x B NB)
 * 1 <= S <= 255, 1 <= Cg <= 4, 1 <= NB <= 16 and B, HW >= 1, else -1; B NB > 65535 or sizes beyond the index ranges: -2; plan null: -3. */
int tmg_ens_spod_plan(const int64_t* dims, int64_t* plan);

/* tmg_ens_spod_csd: csd_raw [B][NB][2][R][R] fp32 from acc and cst (device), bins (NB host integers, 1 <= k < NF) and channels (Cg
 * distinct host integers in 0..C-1), the sums over the Cg HW elements in the order of the plan:
 *   raw0[m][n] = sum Re_m Re_n + sum Im_m Im_n,  raw1[m][n] = sum Re_m Im_n - sum Re_n Im_m          (one fp32 addition each)
 * so that raw0 is bitwise symmetric and raw1 bitwise antisymmetric with a zero diagonal.  ws: the workspace of dims[8] floats, at
 * least the plan's (else -1); written before it is read.  dims = {S, B, C, HW, NF, Tn, NB, Cg, ws_floats}.  Codes as the plan's, and
 * 2 <= C <= 4, NF >= 2, Tn >= 2, valid bins and channels, else -1; a null pointer: -3. */
int tmg_ens_spod_csd(const void* acc, const void* cst, const int64_t* bins, const int64_t* channels, void* ws, void* csd_raw,
                     const int64_t* dims, tmg_stream_t st);

/* tmg_ens_spod_modes: modes [B][NB][2 J][Cg][HW] fp32, row r of (b, bin) = sum_q w[b][bin][r][q] Z_q with the contraction index
 * q < SP: Re X_q, else Im X_{q - SP}, SP = S rounded up to 4 (the padding terms are exact zeros; the target row takes no part), one
 * fmaf chain in q order per output element.  w [B][NB][16][2 SP] device floats (rows >= 2 J are read and must be finite; their
 * products are not stored).  dims = {S, B, C, HW, NF, Tn, NB, Cg, J}, 1 <= J <= 8.  Codes as tmg_ens_spod_csd. */
int tmg_ens_spod_modes(const void* acc, const void* cst, const int64_t* bins, const int64_t* channels, const void* w, void* modes,
                       const int64_t* dims, tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
