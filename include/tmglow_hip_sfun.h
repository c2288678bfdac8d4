/* Structure functions and variogram score of the ensemble members (tmg_sfun.hip: the increments of every member at a list of pixel
 * lags, partials in a workspace, no float atomics: bitwise reproducible).  Included by tmglow_hip.h (which defines tmg_stream_t): do
 * not include it on its own.
 *
 * Setting.  Case b, kept step t, channel c.  Rows x_0..x_{S-1} are the raw normalised members.  Row x_S = y is the normalised target.
 * a_c = u[b,c] * out_std[c] > 0.  out_mu cancels and is not an input.
 * Lags.  A lag is l = (dx, dy) in pixels, dx along W and dy along H.  Lags are in canonical form: dx >= 0, and dy > 0 when dx == 0.
 * 0 <= dx <= 64, |dy| <= 64, dx < W, |dy| < H.  Lags are distinct, with 1 <= L <= 16 of them.  The pairs of a lag are all pixels
 * p = (i, j) for which p' = (i + dy, j + dx) lies in the field.  N_l = (H - |dy|) (W - dx) >= 1.  D_m(p) = x_m(p') - x_m(p).
 * Raw moment sums.  Per row m = 0..S and lag: M_q[m] = sum_p D_m(p)^q for q = 2, 3, 4, in fp32.
 * Raw variogram sum.  Per lag, of order 1/2: s_m(p) = sqrtf(|D_m(p)|); sbar(p) = (s_0 + .. + s_{S-1}, added sequentially in member
 * order in fp32) * fl(1/S); V_l = sum_p (s_S(p) - sbar(p))^2.
 * Physical outputs (formed by the caller from the raw sums in fp64 and rounded once to float32): sf_q = a_c^q M_q / N_l,
 * vario_lag = w_l a_c V_l / N_l with weights w_l > 0. */
#ifndef TMGLOW_HIP_SFUN_H
#define TMGLOW_HIP_SFUN_H

/* tmg_ens_sfun_plan launches nothing: the launch plan of tmg_ens_sfun_step for dims = {S, B, C, H, W, L} and lags [L][2] = (dx, dy)
 * host integers, which the launch body itself calls.  plan (8 + 5 * 16 host integers) = {P, Lc, ws, SL, threads, L, R, 0}, then per
 * lag slot l = 0..15 {off, jmax, ilo, ihi, N} (zeros behind the last lag):
 *   P, SL  pixel slices: slice s = the pixels i W + j in [s SL, min(H W, (s + 1) SL)), SL a multiple of 256 and, for more than one
 *          slice, at least 512; chosen so that B C P blocks fill the device while ws stays under 2^24 floats
 *   threads  = 256: thread t of a block walks the pixels t, t + 256, .. of its slice
 *   a pair (p, p') is counted by the thread that walks p, when j < jmax, ilo <= i < ihi; then p' = p + off, off = dy W + dx;
 *          N = (H - |dy|) (W - dx) is the number of such pixels
 *   P      the partials added per output, in slice order
 *   Lc     = SL / 256 + 9: the fp32 additions along the longest path inside one partial (a thread's SL / 256 terms in order, a
 *          six-deep butterfly over the wave, the four waves in wave order)
 *   R      = S + 1 rows;  ws  floats of workspace: B C P L (3 R + 1) (the moments' partials [B C][R][P][3][L], then the
 *          variogram's [B C][P][L])
 * 2 <= C <= 4, S, B, H, W >= 1, 1 <= L <= 16 and valid lags, else -1; S > 1024, B C > 65535 or sizes beyond the index ranges: -2;
 * lags or plan null: -3. */
int tmg_ens_sfun_plan(const int64_t* dims, const int64_t* lags, int64_t* plan);

/* tmg_ens_sfun_step runs once per kept step, after tmg_ens_score_store has stored the step's S members in xs [S][B][C][HW] (raw
 * normalised values).  target: [B][HW] pixels of C fp32 channels, pixel stride t_d[0], channel offset t_d[1] (normalised, as the
 * members): row S.  Writes the raw sums mom [3][B][C][L][S + 1] (M_2, M_3, M_4; the target's row last) and vsum [B][C][L] (V_l).
 * flags & 1: tmom [3][B][C][L][S + 1] += mom and tvar [B][C][L] += vsum, one fp32 addition per step (t_before = 0: written, not read),
 * t_before the steps they hold.  ws: the workspace of ws_floats floats, at least the plan's (else -1); it is written before it is
 * read.  Non-finite members are not supported.
 * dims = {S, B, C, H, W, L, t_before, flags}.  Codes as tmg_ens_sfun_plan, and t_before >= 0, t_d[0] >= t_d[1] + C, else -1; a null
 * pointer (tmom, tvar only with flags & 1): -3. */
int tmg_ens_sfun_step(const void* xs, const void* target, const int64_t* t_d, const int64_t* lags, void* ws, int64_t ws_floats, void* mom,
                      void* vsum, void* tmom, void* tvar, const int64_t* dims, tmg_stream_t st);

#endif
