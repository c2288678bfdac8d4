/* Energy score and member distances of the ensemble members as whole fields (tmg_gram.hip: a Gram matrix over the pixels on the fp32
 * matrix pipe, partials in a workspace, no float atomics: bitwise reproducible).  Included by tmglow_hip.h (which defines
 * tmg_stream_t): do not include it on its own. */
#ifndef TMGLOW_HIP_GRAM_H
#define TMGLOW_HIP_GRAM_H

/* tmg_ens_gram_plan launches nothing: the launch plan of tmg_ens_gram_step for dims = {S, B, C, HW}, which the launch body itself
 * calls.  plan (7 host integers) = {P, L, NP, ws, SL, NT, part}:
 *   NT  row macro-tiles of 64 rows over the R = S + 1 rows (S members, then the target); NP = NT (NT + 1) / 2 macro-tile pairs I <= J,
 *       pair (I, J) at index I NT - I (I - 1) / 2 + (J - I); only the upper triangle is computed
 *   P   pixel slices, slice s = pixels [s SL, min(HW, (s + 1) SL)), SL a multiple of 256; chosen so that B C NP P blocks fill the
 *       device while ws stays under 2^24 floats (P = 1 may exceed that: ws = B C NP part then)
 *   L   = SL: the fmaf terms of one partial (four waves' chains of SL / 4 end to end, then 3 additions in wave order): L P >= HW
 *   part  floats of one partial: 4096 (a 64 x 64 macro-tile pair), or 256 when S + 1 <= 16 (one 16-row tile: the small instance)
 *   ws  floats of workspace: B C NP part (P + 1) for P > 1 (the partials, then their sums in slice order), B C NP part for P = 1
 * 2 <= C <= 4 and S, B, HW >= 1, else -1; S > 1024, B C > 65535 or sizes beyond the index ranges: -2; plan null: -3. */
int tmg_ens_gram_plan(const int64_t* dims, int64_t* plan);

/* tmg_ens_gram_step runs once per kept step, after tmg_ens_score_store has stored the step's S members in xs [S][B][C][HW] (raw
 * normalised values).  target: [B][HW] pixels of C fp32 channels, pixel stride t_d[0], channel offset t_d[1] (normalised, as the
 * members): row S.  Per case b:
 *   r [B][C][HW] (caller-owned, written): the members' mean, (x_0 + .. + x_{S-1} sequentially in fp32) * fl(1 / S)
 *   e_m = x_m - r (m = 0..S), G_c[m][n] = sum_p e_m e_n per channel c
 *   group g = the channels grp[4 g + 0..3] (host integers, -1 behind the last; 1 <= Gn <= 4 groups, non-empty, every channel in at
 *   most one group): d2_g[m][n] = max(0, sum_{c in g} a2[b][c] (G_c[m][m] + G_c[n][n] - 2 G_c[m][n])), 0 on the diagonal;
 *   a2 [B][C] device floats, the squared un-normalisation scale (u out_std)^2.  dist = sqrt(d2).
 *   outf [5][B][Tk][Gn] at (b, t, g): energy_score = target_dist_mean - pair_dist_mean / 2, energy_score_fair (1 / (S (S - 1)) for
 *   1 / S^2 on the pair sum; S = 1: the pair term is 0), target_dist_mean = (1 / S) sum_{m<S} dist[m][S], pair_dist_mean = (2 / S^2)
 *   sum_{m<n<S} dist[m][n], nearest_dist; the sums in fp64, rounded once.  outi [2][B][Tk][Gn] int64: medoid = argmin_{m<S} sum_{n<S}
 *   dist[m][n], nearest = argmin_{m<S} dist[m][S], ties to the lowest member.
 *   flags & 1: traj [B][Gn][S + 1][S + 1] += d2 (fp32; t_before = 0: written, not read), t_before the steps it holds.
 * ws: the workspace of ws_floats floats, at least the plan's (else -1); it is written before it is read.
 * dims = {S, B, HW, C, Gn, Tk, t, t_before, flags}.  Codes as tmg_ens_gram_plan, and 0 <= t < Tk, t_before >= 0, t_d[0] >= t_d[1] + C,
 * valid groups, else -1; a null pointer (traj only with flags & 1): -3. */
int tmg_ens_gram_step(const void* xs, const void* target, const int64_t* t_d, const void* a2, const int64_t* grp, void* r, void* ws,
                      int64_t ws_floats, void* traj, void* outf, void* outi, const int64_t* dims, tmg_stream_t st);

/* tmg_ens_gram_traj: the same scores and argmins on dist = sqrt(traj) of traj [B][Gn][S + 1][S + 1] (the squared distances between
 * whole roll-outs that tmg_ens_gram_step accumulated): outf [5][B][Gn], outi [2][B][Gn] in the order above.  dims = {S, B, Gn}. */
int tmg_ens_gram_traj(const void* traj, void* outf, void* outi, const int64_t* dims, tmg_stream_t st);

#endif
