/* The budget of the turbulent kinetic energy of the ensemble members and of the target (tmg_budget.hip): time sums of products of every
 * row's own fluctuations about the target's time mean, then production, convection, turbulent transport, pressure diffusion, viscous
 * diffusion, dissipation and their sum in fp64.  No atomics, no LDS, no workspace: bitwise reproducible for every chunking.  A header
 * of its own: tmglow_hip.h (which defines tmg_stream_t) does not include it. */
#ifndef TMGLOW_HIP_BUDGET_H
#define TMGLOW_HIP_BUDGET_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_budget_plan launches nothing: the launch plan of tmg_ens_budget_accum for dims = {S, B, H, W}, which the launch body itself
 * calls.  plan (4 host integers) = {TILE, NT, vec, ws}:
 *   TILE  pixels of one block (256 threads): 1024 on the vector path (4 consecutive pixels of one field row per thread), else 256
 *   NT    = ceil(H W / TILE) blocks per field; the grid is NT x B; block i covers the pixels [i TILE, min(HW, (i + 1) TILE)) once
 *   vec   1: the planes of raw are read and written with 16-byte accesses, which a call takes when W % 4 == 0 AND the base of raw is
 *         16-byte aligned; the plan assumes an aligned base, so vec = (W % 4 == 0).  The input rows are read with dword loads on
 *         both paths, so dense rows and channel slices take the same path
 *   ws    workspace floats: always 0
 * S, B >= 1 and H, W >= 3, else -1; S > 1024, B > 65535 or sizes beyond the index ranges: -2; a null pointer: -3. */
int tmg_ens_budget_plan(const int64_t* dims, int64_t* plan);

/* tmg_ens_budget_accum: rows [k B][H W] pixels of 3 fp32 channels (ux, uy, p), pixel stride t_d[0], channel offset t_d[1] (raw
 * normalised values; row s B + b is member row0 + s of case b; the target is fed as k = 1, row0 = S).  Device tables: a [B][3] the
 * scales, m [B][3][HW] the target's time mean (normalised; null: 0).  raw [S + 1][B][14][HW] fp32.  With d_c = fl(a_c fl(x_c - m_c)),
 * f = 0 outside the field,
 *   Sx f = fl(fl(fl(f[h-1,w+1] - f[h-1,w-1]) + fl(2 fl(f[h,w+1] - f[h,w-1]))) + fl(f[h+1,w+1] - f[h+1,w-1]))
 *   Sy f = fl(fl(fl(f[h+1,w-1] - f[h-1,w-1]) + fl(2 fl(f[h+1,w] - f[h-1,w]))) + fl(f[h+1,w+1] - f[h-1,w+1]))
 * the terms of the 14 planes are d_u, d_v, d_p; fl(d_u d_u), fl(d_u d_v), fl(d_v d_v); fl(fl(d_u d_u) d_u), fl(fl(d_u d_u) d_v),
 * fl(fl(d_u d_v) d_v), fl(fl(d_v d_v) d_v); fl(d_p d_u), fl(d_p d_v); fl(fl(Sx d_u Sx d_u) + fl(Sx d_v Sx d_v)); the same with Sy.
 * raw[row][b][q] = fl(raw + term) (fp32, no contraction); with t_before == 0 the term is stored instead, so raw needs no memset.
 * An element is touched by one thread, once per call.  dims = {k, S, B, H, W, row0, t_before}.  Codes as tmg_ens_budget_plan, and
 * k >= 1, 0 <= row0, row0 + k <= S + 1, t_before >= 0, t_d[0] >= t_d[1] + 3, t_d[1] >= 0, else -1. */
int tmg_ens_budget_accum(const void* rows, const int64_t* t_d, const void* a, const void* m, void* raw, const int64_t* dims,
                         tmg_stream_t st);

/* tmg_ens_budget_terms: raw as above after T timed steps; M [B][2][HW] fp64 the target's physical mean velocity; fl (4 HOST doubles)
 * = {dx, dy, nu, rho}, dx, dy, rho > 0, nu >= 0, finite.  Per row, in fp64, with D_c = raw_c / T: the central moments
 *   uu = raw_3 / T - D_u^2, uv, vv;  uuu = raw_6 / T - 3 D_u raw_3 / T + 2 D_u^3;
 *   uuv = raw_7 / T - 2 D_u raw_4 / T - D_v raw_3 / T + 2 D_u^2 D_v, uvv, vvv likewise;  pu = raw_10 / T - D_p D_u, pv;
 *   gx = raw_12 / T - (Sx D_u)^2 - (Sx D_v)^2, gy;  k = (uu + vv) / 2;  U = M_u + D_u, V = M_v + D_v;  dx f = Sx f / (8 dx), dy f = Sy f / (8 dy)
 * and the seven terms, in this order:
 *   conv = -(U dx k + V dy k);  prod = -(uu dx U + uv (dy U + dx V) + vv dy V);  turb = -(dx (uuu + uvv) + dy (uuv + vvv)) / 2;
 *   pres = -(dx pu + dy pv) / rho;  visc = nu ((k[h,w+1] - 2 k + k[h,w-1]) / dx^2 + (k[h+1,w] - 2 k + k[h-1,w]) / dy^2);
 *   diss = -nu (gx / (64 dx^2) + gy / (64 dy^2));  resid = the sum of the six.
 * Every term is NaN on the one-pixel frame of the field.  Outputs (fp32): budget_mean, budget_std [B][7][HW] the Welford mean and
 * population std over the S members in member order, target_budget [B][7][HW] row S's; stress_mean, stress_std, target_stress
 * [B][3][HW] the same of uu, uv, vv (defined on the whole field); member_budget [B][S][7][HW] every member's terms, or null.
 * dims = {S, B, H, W, T}.  Codes as tmg_ens_budget_plan, and T >= 1 and a valid fl, else -1. */
int tmg_ens_budget_terms(const void* raw, const void* M, const double* fl, void* budget_mean, void* budget_std, void* target_budget,
                         void* stress_mean, void* stress_std, void* target_stress, void* member_budget, const int64_t* dims,
                         tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
