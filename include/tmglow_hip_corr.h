/* Two-point space-time correlations of the ensemble members and of the target about probe points (tmg_corr.hip):
 *   R(x0; x, tau) = < u'_i(x0, t) u'_j(x, t + tau) >
 * from time sums of products of every row's own fluctuations about the target's time mean, then the covariance and the Pearson
 * coefficient in fp64.  No atomics, no LDS, no workspace: bitwise reproducible for every chunking.  A header of its own: tmglow_hip.h
 * (which defines tmg_stream_t) does not include it.
 *
 * cfg (HOST integers, the same array for the three launches) = {P, Q, L, h_0, w_0, .., h_{P-1}, w_{P-1}, ci_0, cj_0, .., ci_{Q-1},
 * cj_{Q-1}, tau_0, .., tau_{L-1}}: P <= 8 probe pixels inside the field (duplicates allowed), Q <= 4 pairs of channels in 0..2 (ci at
 * the probe, cj in the field), L <= 8 strictly increasing lags in timed steps, tau_0 = 0, tau_{L-1} <= 64.  J is the sorted set of
 * distinct cj.  Rows are the S members plus the target as row S; d_c = fl(a_c fl(x_c - m_c)).
 *
 * State: series [S + 1][B][steps][P][3] fp32, every row's d at the probe pixels at every timed step, and raw [S + 1][B][NPL][HW] fp32
 * with NPL = P Q L + 2 |J| L planes:
 *   X[p,q,l] at plane (p Q + q) L + l            += fl(series[row][b][t - tau_l][p][ci_q] * d_{cj_q}(x, t))
 *   F[j,l]   at plane P Q L + j L + l            += d_j(x, t)
 *   G[j,l]   at plane P Q L + |J| L + j L + l    += fl(d_j d_j)
 * A plane of lag l is updated at the timed steps t >= tau_l only and stored instead of added at t == tau_l, so raw needs no memset;
 * a lag with tau_l >= T leaves its planes unwritten, and they are never read. */
#ifndef TMGLOW_HIP_CORR_H
#define TMGLOW_HIP_CORR_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_corr_plan launches nothing: the launch plan of tmg_ens_corr_accum for dims = {S, B, H, W, P, Q, L, |J|}, which the launch
 * bodies themselves call.  plan (8 host integers) = {TILE, NT, vec, NPL, offX, offF, offG, ws}:
 *   TILE  pixels of one block (256 threads): 1024 on the vector path (4 consecutive pixels of one field row per thread), else 256
 *   NT    = ceil(H W / TILE) blocks per field; the grid is NT x B; block i covers the pixels [i TILE, min(HW, (i + 1) TILE)) once
 *   vec   1: the planes of raw are read and written with 16-byte accesses, which a call takes when W % 4 == 0 AND the base of raw is
 *         16-byte aligned; the plan assumes an aligned base, so vec = (W % 4 == 0)
 *   NPL   = P Q L + 2 |J| L planes; offX = 0, offF = P Q L, offG = P Q L + |J| L the first plane of each kind;  ws = 0
 * S, B, H, W, P, Q, L, |J| >= 1 and |J| <= min(Q, 3), else -1; S > 1024, B > 65535, P > 8, Q > 4, L > 8 or sizes beyond the index
 * ranges: -2; a null pointer: -3. */
int tmg_ens_corr_plan(const int64_t* dims, int64_t* plan);

/* tmg_ens_corr_probe: rows [k B][H W] pixels of 3 fp32 channels, pixel stride t_d[0], channel offset t_d[1] (row s B + b is member
 * row0 + s of case b; the target: k = 1, row0 = S).  Device tables: a [B][3], m [B][3][HW] (null: 0).  One thread per (row of the
 * chunk, case, probe, channel) writes series[row0 + s][b][t][p][c] = fl(a_c fl(x_c - m_c)) at the probe's pixel.  Launched before
 * tmg_ens_corr_accum on the same stream.  dims = {k, S, B, H, W, row0, t, steps}.  Codes as tmg_ens_corr_plan, and k >= 1,
 * 0 <= row0, row0 + k <= S + 1, 0 <= t < steps, t_d[0] >= t_d[1] + 3, t_d[1] >= 0 and a valid cfg, else -1. */
int tmg_ens_corr_probe(const void* rows, const int64_t* t_d, const void* a, const void* m, void* series, const int64_t* cfg,
                       const int64_t* dims, tmg_stream_t st);

/* tmg_ens_corr_accum: rows, t_d, a, m and dims as tmg_ens_corr_probe; series as written by it for these rows at the timed steps
 * 0 .. t.  A thread owns one pixel, or four consecutive pixels of a field row on the vector path, and loops over the chunk's k rows:
 * it forms d once per row and walks the live planes (tau_l <= t) in groups of up to 16; all loads of a group are issued before its
 * arithmetic and its stores come last.  raw = fl(raw + term), fp32, no contraction, one addition per timed step in step order; at
 * t == tau_l the term is stored.  The lag gate and the store-or-add choice are uniform across the launch.  An element of raw is
 * touched by one thread, once per call. */
int tmg_ens_corr_accum(const void* rows, const int64_t* t_d, const void* a, const void* m, const void* series, void* raw,
                       const int64_t* cfg, const int64_t* dims, tmg_stream_t st);

/* tmg_ens_corr_finalize: raw as above after T timed steps; pm, pv [S + 1][B][P][Q][L] fp64 DEVICE tables, the mean and the
 * population variance of series[row][b][0 .. n_l - 1][p][ci_q], n_l = T - tau_l.  One thread per (case, pixel), in fp64, per
 * (p, q, l) and row with n = n_l, j the index of cj_q in J:
 *   mf = F[j,l] / n;  vf = G[j,l] / n - mf^2;  cov = X[p,q,l] / n - pm mf;  rho = cov / sqrt(pv vf) when pv > 0 and vf > 0, else NaN
 * (the Pearson coefficient of the n paired samples).  Lags with n_l < 2 give NaN and read no plane.  Outputs (fp32):
 *   cov_mean, cov_std, rho_mean, rho_std [B][P][Q][L][HW]  the Welford mean and population std over the S members in member order
 *   target_cov, target_rho [B][P][Q][L][HW]                row S
 *   member_rho [B][S][P][Q][L][HW]                         every member's rho, or null
 *   line_x [B][S + 1][P][Q][L][W], line_y [B][S + 1][P][Q][L][H]   rho of every row on the probe's field row and field column
 * dims = {S, B, H, W, T}.  Codes as tmg_ens_corr_plan, and T >= 1 and a valid cfg, else -1. */
int tmg_ens_corr_finalize(const void* raw, const void* pm, const void* pv, void* cov_mean, void* cov_std, void* rho_mean,
                          void* rho_std, void* target_cov, void* target_rho, void* member_rho, void* line_x, void* line_y,
                          const int64_t* cfg, const int64_t* dims, tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
