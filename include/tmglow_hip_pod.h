/* Projection of the ensemble members and of the target on the target's POD modes (tmg_pod.hip: per case a [rows x pixels channels] by
 * [pixels channels x K] product on the fp32 matrix pipe straight from the chunk's NHWC rows, partials in a workspace, no float
 * atomics: bitwise reproducible for every chunking).  Included by tmglow_hip.h (which defines tmg_stream_t): do not include it on
 * its own. */
#ifndef TMGLOW_HIP_POD_H
#define TMGLOW_HIP_POD_H

/* tmg_ens_pod_plan launches nothing: the slice plan of tmg_ens_pod_project for dims = {S, B, Cg, HW, K}, which the launch body itself
 * calls.  plan (4 host integers) = {P, SL, L, ws}:
 *   P   pixel slices, slice s = pixels [s SL, min(HW, (s + 1) SL)), SL a multiple of 256 (four waves x one chunk of 64 pixels):
 *       P = min(ceil(HW / 256), 32), SL = ceil(HW / P) rounded up to 256, then P = ceil(HW / SL).  P and SL depend on HW alone, never
 *       on the rows of the call: a member's sums are the same bits in every chunk it may be fed in
 *   L   = SL Cg: the fmaf terms of one partial (the four waves' chains of SL Cg / 4 end to end; they are added in wave order, 3
 *       additions, and the energy's four pixel-group chains in group order, 3 more): L P >= HW Cg
 *   ws  floats of workspace for a call of S members (S B rows): P S B 17 for P > 1 (per slice and row the 16 mode sums, then the
 *       energy sum; folded in slice order by a second kernel), 0 for P = 1 (the block writes the outputs itself)
 * S, B, HW >= 1, 1 <= Cg <= 4, 1 <= K <= 16, else -1; S > 1024, B > 65535 or sizes beyond the index ranges: -2; a null pointer: -3. */
int tmg_ens_pod_plan(const int64_t* dims, int64_t* plan);

/* tmg_ens_pod_project: rows [k B][HW] pixels of fp32 channels, pixel stride t_d[0], channel offset t_d[1] (raw normalised values; row
 * s B + b is member s of case b: a chunk of k members, or the B target rows with k = 1).  ch: the Cg distinct channels (host integers,
 * 0 <= ch < t_d[0] - t_d[1]).  Device tables: a [B][Cg] the scales, m [B][Cg][HW] the mean planes, psi [B][K][Cg][HW] the modes.
 * Per row, with d = fl(a fl(x - m)) (two fp32 roundings, no contraction):
 *   coef_raw[j] = sum_c sum_p d psi_j (j < K),  en_raw = sum_c sum_p d d      fp32 fmaf chains in the order of the plan
 * written at coef + b o_d[0] + s o_d[1] + j and en + b o_d[2] + s o_d[3] (element strides of the caller's [B, S, Tk, ..] outputs, the
 * pointers already at member m0 and step t).  Rows beyond k B, modes beyond K and pixels beyond HW contribute exact zeros.
 * ws: the workspace of ws_floats floats, at least the plan's for S = k (else -1); it is written before it is read.
 * dims = {k, B, HW, Cg, K}.  Codes as tmg_ens_pod_plan, and t_d[0] >= t_d[1] + 1, valid distinct channels, strides >= 0, else -1; a
 * null pointer (ws only when the plan needs one): -3. */
int tmg_ens_pod_project(const void* rows, const int64_t* t_d, const int64_t* ch, const void* a, const void* m, const void* psi, void* ws,
                        int64_t ws_floats, void* coef, void* en, const int64_t* o_d, const int64_t* dims, tmg_stream_t st);

#endif
