/* One-dimensional line spectra of the ensemble members (tmg_lspec.hip): per line of the field the one-sided autospectra of the
 * channels and the co- and quadrature spectrum of channels 0 and 1, of every step (total), of each member's time-mean coefficient
 * (mean flow) and of its fluctuation about that mean, in ONE pass over the roll-out.  No atomics; every element of every state is
 * owned by one lane and every sum has a fixed order, so every output is bitwise reproducible and independent of the chunking.  A
 * header of its own: tmglow_hip.h (which defines tmg_stream_t) does not include it.
 *
 * THE DEFINITIONS.  A line is a row (axis x: L = H lines of N = W points) or a column (axis y: L = W lines of N = H points) of an
 * image; the kernels see only (L, N, line stride, point stride) in pixels.  Per case b, member, step, channel c < C and line l:
 *   yh = u[b,c] * fmaf(out_std[c], y_c, out_mu[c])               the physical value (tmg_unnorm_fma)
 *   X_c[l,q] = sum_n op[n][q] yh_c[l,n]     q = 0 .. N/2         op: the host-built operand [2][N][NQP] (re, im), NQ = N/2 + 1 padded
 *                                                                to NQP = 16 ceil(NQ / 16) with zero columns,
 *                                                                op[n][q] = (w[n] / N) exp(-2 pi i ((q n) mod N) / N) built in fp64 and
 *                                                                rounded once; the products run on the fp32 matrix pipe, n ascending
 *   planes f = 0 .. F-1, F = C + 2: |X_c|^2 (c = 0 .. C-1), co = Re(X_0 conj X_1) = r0 r1 + i0 i1, quad = Im(X_0 conj X_1) = i0 r1 - r0 i1
 *   a_q = 1 at q = 0 and q = N/2, else 2 (exact in fp32, applied where a plane leaves the state)
 * Total spectrum of a step: a_q times the planes of X, averaged over the L lines.  Mean-flow spectrum of a member: a_q times the
 * planes of Xbar, its running mean over the timed steps.  Fluctuation spectrum of a member: a_q M / T with the co-moment
 *   M_xy += (X_t - Xbar_{t-1}) conj(Y_t - Ybar_t)                (Welford; never mean|X|^2 - |Xbar|^2)
 * A member's first timed step stores its state without reading it; T = 1 leaves M exactly 0.
 * Non-finite members are not supported: the outputs they touch are unspecified; no address depends on the data. */
#ifndef TMGLOW_HIP_LSPEC_H
#define TMGLOW_HIP_LSPEC_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_lspec_plan launches nothing: dims = {k, S, B, C, L, N} -> out (12 host integers) = {tiles, mode_tiles, grid_x, grid_y,
 * threads, lds_bytes, nq, nqp, part_floats, mean_floats, comom_floats, operand_floats}:
 *   tiles          = ceil(L / 16): the 16-line tiles of an image, the last one masked
 *   mode_tiles     = nqp / 16: the 16-mode tiles the four waves of a block share out
 *   chunk grid     = (tiles, k B), 256 threads; lds_bytes = 64 C (N + 4): C channels of 16 lines, line stride N + 4 floats
 *   part_floats    = k B tiles F nq: the tiles' line sums of the total planes [k B][tiles][F][nq]
 *   mean_floats    = 2 S B C L nq, comom_floats = S B F L nq: the members' state (44 S B L nq bytes at C = 3)
 *   operand_floats = 2 N nqp
 * k, S, B, L >= 1, C in 2 .. 4, N a multiple of 16 in [16, 512], k <= S, else -1; S > 1024, k B > 65535, ceil(L / 16) > 65535 or a
 * state beyond 2^31 floats: -2; a null pointer: -3. */
int tmg_ens_lspec_plan(const int64_t* dims, int64_t* out);

/* tmg_ens_lspec_chunk transforms the lines of the k B images (rows member-major) of the NHWC chunk y (y_d = {pixel stride, channel
 * offset}: dense rows and channel-slice views).  dims = {k, S, B, C, L, N, line stride, point stride, m0, t_before, flags,
 * part_floats, mean_floats, comom_floats, operand_floats}; the strides are in pixels, (W, 1) for rows and (1, W) for columns of an
 * image of L N pixels.  u [B][C] or null (1), out_mu / out_std [C], op: the operand above.
 *   flags & 1 (a timed step): the running mean [S][B][C][L][nq][2] and the co-moments [S][B][F][L][nq] of the members m0 .. m0 + k - 1
 *     take one more step; t_before = 0 stores them without reading.  Without the flag neither is touched and both may be null.
 *   always: part [k B][tiles][F][nq] = the tile's sum over its lines of the planes of X (no a_q), lines in a fixed order.
 * Codes: the plan's; strides that are not (1, L) or (N, 1) with a point stride >= 1, a descriptor that does not hold C channels,
 * m0 < 0, m0 + k > S, t_before < 0, flags outside 0 .. 1: -1; a chunk beyond the index range: -2; a null pointer among those the
 * flags make it touch: -3; a buffer under the plan's size: -4.  Every code comes before the launch. */
int tmg_ens_lspec_chunk(const void* y, const int64_t* y_d, const void* u, const void* out_mu, const void* out_std, const void* op,
                        void* mean, void* comom, void* part, const int64_t* dims, tmg_stream_t st);

/* tmg_ens_lspec_step folds one chunk's partial sums into the step's statistics over the members: per (case, plane, mode) the tiles
 * in tile order, times a_q, over L; then a SEQUENTIAL Welford over the members that continues from the stored (mean, M2) of
 * state [2][B][F][nq] (n_before = 0: it starts at 0 without reading), so that every chunking gives the same bits.  last = 1: the
 * mean and the population std go to mean_out / std_out [B][Tk][F][nq] at step t instead of the state.
 * dims = {k, B, F, L, N, n_before, S, Tk, t, last}.  Codes: a size under 1, F outside 4 .. 6, N off the grid, t outside 0 .. Tk - 1,
 * last = 1 with n_before + k != S (or 0 with it equal), n_before + k > S: -1; B F > 65535 or S > 1024: -2; a null pointer among
 * those touched: -3. */
int tmg_ens_lspec_step(const void* part, void* state, void* mean_out, void* std_out, const int64_t* dims, tmg_stream_t st);

/* tmg_ens_lspec_finalize: per (case, plane, line, mode) the mean and population std over the members, in member order (Welford), of
 * the fluctuation spectrum a_q M / T and of the mean-flow spectrum a_q planes(Xbar), into fluct_mean, fluct_std, flow_mean, flow_std
 * [B][F][L][nq]; member_out [B][S][F][L][nq] or null: every member's fluctuation spectrum.  dims = {S, B, C, L, N, T}.
 * Codes: a size under 1, C outside 2 .. 4, N off the grid: -1; S > 1024 or a state beyond 2^31 floats: -2; a null pointer (but
 * member_out): -3. */
int tmg_ens_lspec_finalize(const void* mean, const void* comom, void* fluct_mean, void* fluct_std, void* flow_mean, void* flow_std,
                           void* member_out, const int64_t* dims, tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
