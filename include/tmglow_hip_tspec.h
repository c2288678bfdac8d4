/* Temporal power spectra of the ensemble members (tmg_tspec.hip; no atomics: bitwise reproducible).  Included by tmglow_hip.h (which
 * defines tmg_stream_t): do not include it on its own. */
#ifndef TMGLOW_HIP_TSPEC_H
#define TMGLOW_HIP_TSPEC_H

/* Per element e of [S][B][C][HW] (member, case, channel, pixel; E = S B C HW of them) the series xh_n = u[b][c] (out_std[c] y_n +
 * out_mu[c]) over the Tn fed steps, d_n = g_n (xh_n - xbar), X_k = sum_n d_n exp(-2 pi i k n / Tn), P_k = c_k |X_k|^2 / Tn^2 for
 * k = 0 .. NF - 1.  Blocked in time: a planar ring [16][E] takes 16 steps, then one pass folds them into the accumulator acc [R][E],
 * R = 2 NF + 1 rows: re_k at row k, im_k at row NF + k, the plain sum of xh at row 2 NF.
 *
 * tmg_tspec_store un-normalises one chunk of k members into rows m0 .. m0 + k - 1 of ring slot `slot`.  y, y_d and the row order as
 * tmg_ens_accum (row j*B + b = member m0 + j, case b; y_d = {pixel stride, channel offset}); u: [B][C] or NULL for 1; out_mu, out_std:
 * C floats.  dims = {k, B, HW, C, S, m0, slot}; 2 <= C <= 4, m0 + k <= S, 0 <= slot < 16, else -1; sizes beyond the index ranges: -2;
 * a null pointer: -3. */
int tmg_tspec_store(const void* y, const int64_t* y_d, const void* u, const void* out_mu, const void* out_std, void* ring,
                    const int64_t* dims, tmg_stream_t st);
/* tmg_tspec_block folds the nb <= 16 valid ring slots 0 .. nb - 1, which hold steps n0 .. n0 + nb - 1, into acc on the fp32 matrix
 * pipe: acc[r][e] (+)= sum_j tm[n0 + j][r] ring[j][e].  tm: the operand [Tn][RP] floats, RP = R rounded up to 16, columns >= R zero.
 * Slots >= nb are neither read nor multiplied.  first != 0: acc is written, else added to.  dims = {E, Tn, NF, n0, nb, first};
 * 1 <= nb <= 16, n0 + nb <= Tn, NF >= 1, else -1; E >= 2^40 or (2 NF + 1) E >= 2^44: -2; a null pointer: -3. */
int tmg_tspec_block(const void* tm, const void* ring, void* acc, const int64_t* dims, tmg_stream_t st);
/* tmg_tspec_finalize: per member X_k = (re_k, im_k) - xbar G_k with xbar = sum * fl[0] (fl[0] = 1 / Tn), P_k = cst[2][k] |X_k|^2,
 * then mean and population std of P_k over the S members (Welford, in member order) into psd_mean / psd_std [B][NF][C][HW].
 * cst: [3][NF] floats = (Re G_k, Im G_k, c_k / Tn^2).  dims = {S, B, C, HW, NF}; 2 <= C <= 4, else -1; sizes beyond the index
 * ranges: -2; a null pointer: -3. */
int tmg_tspec_finalize(const void* acc, const void* cst, void* psd_mean, void* psd_std, const int64_t* dims, const float* fl,
                       tmg_stream_t st);

#endif
