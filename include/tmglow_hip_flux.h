/* The scale-to-scale energy flux and the sub-filter stresses of the ensemble members and of the target (tmg_flux.hip): the
 * coarse-graining analysis with box filters of L widths, tau_ij = bar(u_i u_j) - bar(u_i) bar(u_j), Pi = -tau_ij d bar(u_i) / dx_j at
 * every instant, summed over the timed steps, then the time means, the temporal std, the backscatter fraction and the headline curves
 * in fp64.  No atomics, no partial sums in the state: bitwise reproducible for every chunking.  A header of its own: tmglow_hip.h
 * (which defines tmg_stream_t) does not include it.
 * widths (L HOST integers, 1 <= L <= 8): odd box widths w in 3 .. 33 pixels, strictly increasing, each <= min(H, W) - 2.  r = w / 2,
 * N = w^2.  A pixel (h, w) is valid for a width when r + 1 <= h <= H - 2 - r and r + 1 <= w <= W - 2 - r. */
#ifndef TMGLOW_HIP_FLUX_H
#define TMGLOW_HIP_FLUX_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_flux_plan launches nothing: the launch plan of tmg_ens_flux_accum for dims = {S, B, H, W, L} and widths, which the launch
 * body itself calls; a function of (H, W, widths), B only scales the blocks.  plan (8 host integers) =
 * {TH, TW, halo, NTY, NTX, lds, optin, blocks}:
 *   TH, TW    = 32, 32: the tile of one block (1024 threads, a pixel each)
 *   halo      = r_max + 1: the box of the largest width plus the ring of the stencils
 *   NTY, NTX  tiles per direction; they cover the valid region of the smallest width, rows and columns r_0 + 1 .. H - 2 - r_0:
 *             tile (i, j) owns the pixels [r_0 + 1 + 32 i, ..) x [r_0 + 1 + 32 j, ..) of that region, each once
 *   lds       bytes of dynamic LDS of a block: 4 (2 rows 66 + 5 rows 34 + 2 34 34), rows = TH + 2 halo
 *   optin     1 when lds exceeds 64 KB (r_max >= 7): the launch raises the kernel's dynamic LDS limit first
 *   blocks    = NTY NTX B per fed row; the grid of a call with k rows is (NTY NTX, k, B)
 * S, B >= 1, H, W >= 5, valid widths, else -1; S > 1024, B > 65535 or sizes beyond the index ranges: -2; a null pointer: -3. */
int tmg_ens_flux_plan(const int64_t* dims, const int64_t* widths, int64_t* plan);

/* tmg_ens_flux_accum: rows [k B][H W] pixels of fp32 channels of which the first two (ux, uy) are read, pixel stride t_d[0], channel
 * offset t_d[1] (raw normalised values; row s B + b is member row0 + s of case b; the target is fed as k = 1, row0 = S).  Device
 * tables: a [B][2] the scales, kk [L][2] = fl(1 / (8 dx N^3)), fl(1 / (8 dy N^3)).  raw [S + 1][B][L][7][HW] fp32.  With
 * f_c = fl(a_c x_c), the box sums Sg_u, Sg_v, Sg_uu, Sg_uv, Sg_vv of f_u, f_v, fl(f_u f_u), fl(f_u f_v), fl(f_v f_v) over the w x w box
 * centred on the pixel are a row pass, then a column pass, both from the centre outwards:
 *   s_0 = g[0], s_j = fl(fl(s_{j-1} + g[-j]) + g[+j]), j = 1 .. r
 * and, with the stencils applied to the box sums of the eight neighbours,
 *   Sx g = fl(fl(fl(g[h-1,w+1] - g[h-1,w-1]) + fl(2 fl(g[h,w+1] - g[h,w-1]))) + fl(g[h+1,w+1] - g[h+1,w-1]))
 *   Sy g = fl(fl(fl(g[h+1,w-1] - g[h-1,w-1]) + fl(2 fl(g[h+1,w] - g[h-1,w]))) + fl(g[h+1,w+1] - g[h-1,w+1]))
 *   Q_uu = fl(fl(N Sg_uu) - fl(Sg_u Sg_u)), Q_uv = fl(fl(N Sg_uv) - fl(Sg_u Sg_v)), Q_vv = fl(fl(N Sg_vv) - fl(Sg_v Sg_v))
 *   A = fl(fl(Q_uu Sx Sg_u) + fl(Q_uv Sx Sg_v)), B = fl(fl(Q_uv Sy Sg_u) + fl(Q_vv Sy Sg_v)), Pi_s = -fl(fl(A kk_x) + fl(B kk_y))
 * the terms of the 7 planes are A, B, fl(Pi_s Pi_s), [Pi_s < 0], Q_uu, Q_uv, Q_vv.  raw[row][b][l][q] = fl(raw + term) (fp32, no
 * contraction) at the valid pixels of width l; with t_before == 0 the term is stored instead, so raw needs no memset.  Invalid pixels
 * are neither read nor written.  An element is touched by one thread, once per call.
 * dims = {k, S, B, H, W, row0, t_before, L}.  Codes as tmg_ens_flux_plan, and k >= 1, 0 <= row0, row0 + k <= S + 1, t_before >= 0,
 * t_d[0] >= t_d[1] + 2, t_d[1] >= 0, else -1. */
int tmg_ens_flux_accum(const void* rows, const int64_t* t_d, const void* a, const void* kk, void* raw, const int64_t* widths,
                       const int64_t* dims, tmg_stream_t st);

/* tmg_ens_flux_terms: raw as above after T timed steps; k64 [L][2] fp64 on the device = 1 / (8 dx N^3), 1 / (8 dy N^3).  Per row and
 * width, in fp64 at the valid pixels (NaN elsewhere):
 *   Pi = -((raw_0 k64_x + raw_1 k64_y) / T);  tstd = sqrt(max(raw_2 / T - Pi^2, 0));  back = raw_3 / T;  tau = raw_4..6 / ((N N) T)
 * outs (14 HOST pointers to device fp32 arrays), in this order: flux_mean, flux_std, target_flux, tstd_mean, target_tstd, back_mean,
 * back_std, target_back [B][L][HW]; sgs_mean, sgs_std, target_sgs [B][L][3][HW] (uu, uv, vv); member_flux [B][S][L][HW] or null;
 * flux_curve, sgs_curve [B][S + 1][L]: the mean over the width's valid pixels of Pi and of (tau_uu + tau_vv) / 2, per row, the target
 * last.  Means and population stds are Welford over the S members in member order; target_* is row S's.  ws: B (S + 1) L 2 NW doubles
 * on the device, NW = 4 ceil(HW / 256): one partial per wave (xor butterfly), folded in wave order by a second launch.
 * dims = {S, B, H, W, T, L}.  Codes as tmg_ens_flux_plan, and T >= 1, else -1. */
int tmg_ens_flux_terms(const void* raw, const void* k64, void* const* outs, void* ws, const int64_t* widths, const int64_t* dims,
                       tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
