/* Prediction intervals of the ensemble members (tmg_quant.hip; no LDS, no atomics: bitwise reproducible).  Included by tmglow_hip.h
 * (which defines tmg_stream_t): do not include it on its own. */
#ifndef TMGLOW_HIP_QUANT_H
#define TMGLOW_HIP_QUANT_H

/* tmg_ens_quant_step runs once per kept step, after tmg_ens_score_store has stored the step's S members in xs [S][B][C][HW] (raw
 * normalised values x_0 .. x_{S-1} per element).  Per (case b, channel c, pixel p):
 *   rank_m = #{n : x_n < x_m} + #{n < m : x_n == x_m}, a permutation of 0 .. S - 1 (ties broken by member index); the order statistic
 *   x_(r) is the member of rank r.
 *   Q levels j, each given by the host as (lo_j, hi_j, w_j): qraw_j = x_(lo) + w (x_(hi) - x_(lo)), three rounded fp32 operations in
 *   this order (no contraction); quant = sc * fmaf(out_std[c], qraw_j, out_mu[c]) at quant + b * o_d[0] + (j * C + c) * HW + p, with
 *   sc = u[b][c] (u: [B][C], or NULL for 1).  sc * out_std > 0 is the caller's to guarantee: it keeps the order.
 *   K thresholds k, each (channel ex[2k], direction ex[2k + 1]: 1 for x > thr, 0 for x < thr, both strict) with the raw threshold
 *   thr[b * K + k] (device floats): count = #{m : x_m > thr} (or <) over the members of channel ex[2k],
 *   exceed = float(count) * float(1 / S) at exceed + b * o_d[1] + k * HW + p.
 *   flags & 1: the step goes into the time aggregates, which hold t_before steps (t_before = 0: they are written, not read):
 *     tquant [B][Q][C][HW] fp32, m += (quant - m) * (1 / (t_before + 1)); texceed [B][K][HW] int32 += count; and, when flags & 2,
 *     tbelow [B][Q][C][HW] int32 += (y < qraw_j), strict, on the raw values.
 *   flags & 2: a target is given: [B][HW] pixels of C fp32 channels, pixel stride t_d[0], channel offset t_d[1] (normalised, as the
 *     members).  Without it target, t_d and tbelow are not read.
 * lohi: 2 Q host integers (lo_0, hi_0, lo_1, ..), w: Q host floats, ex: 2 K host integers.
 * dims = {S, B, HW, C, Q, K, t_before, flags}.  2 <= C <= 4, 1 <= Q <= 8, 0 <= K <= 4, every lo / hi in 0 .. S - 1, every channel in
 * 0 .. C - 1, every direction 0 or 1, o_d[0] >= Q C HW, o_d[1] >= K HW, t_d[0] >= t_d[1] + C, else -1; S > 1024 or sizes beyond the
 * index ranges: -2; a null pointer among the operands the flags, Q and K require: -3.
 * Non-finite members are not supported: the outputs of a pixel that holds one are unspecified (they may be NaN); no access leaves
 * the buffers and the other pixels are unaffected. */
int tmg_ens_quant_step(const void* xs, const void* target, const int64_t* t_d, const void* u, const void* out_mu, const void* out_std,
                       const int64_t* lohi, const float* w, const void* thr, const int64_t* ex, void* quant, void* exceed, void* tquant,
                       void* tbelow, void* texceed, const int64_t* o_d, const int64_t* dims, tmg_stream_t st);

#endif
