/* Probabilistic event verification of the ensemble members against the target (tmg_event.hip: per-pixel member counts, reliability
 * tables, the raw sums of the fractions skill score over tile-local summed-area tables in LDS; integer adds only, no float atomics:
 * bitwise reproducible).  Included by tmglow_hip.h (which defines tmg_stream_t): do not include it on its own.
 *
 * Setting.  Case b, kept step t.  An event k (1 <= K <= 4) is (channel ev[2k], direction ev[2k + 1]: 1 for x > thr, 0 for x < thr, both
 * strict) with the raw threshold thr[b * K + k] (device floats).  Per pixel p of the H x W field, over the raw normalised members
 * x_0..x_{S-1} and the raw normalised target y of the event's channel:
 *   n = #{m : x_m <> thr} in 0..S,  o = [y <> thr] in {0, 1}.
 * Tables, S + 1 bins: rel_count[j] = #{p : n = j}, rel_hit[j] = #{p : n = j, o = 1}.
 * Neighbourhood sums at an odd width w (1 <= w <= 33, distinct, 1 <= NS <= 8 of them), r = w / 2: Nf(p) = sum of n, No(p) = sum of o
 * over the w x w box centred on p, zeros outside the field.  Raw sums per width, int64: A = sum_p Nf^2, Bx = sum_p Nf No,
 * Cc = sum_p No^2.  S^2 w_max^4 H W < 2^63 keeps them in range. */
#ifndef TMGLOW_HIP_EVENT_H
#define TMGLOW_HIP_EVENT_H

/* tmg_ens_event_plan launches nothing: the launch plan of tmg_ens_event_step's neighbourhood kernel for dims = {S, B, H, W, K, NS}
 * and scales (NS host integers, the widths), which the launch body itself calls.  plan (12 host integers) =
 * {TH, TW, halo, NTY, NTX, lds, threads, ws, pitch, rows, blocks, 0}:
 *   TH, TW    the tile: block (ty, tx) of one (b, k) plane owns the pixels [ty TH, min(H, (ty + 1) TH)) x [tx TW, min(W, (tx + 1) TW))
 *   halo      = the largest w / 2 requested: the block loads rows ty TH - halo .. ty TH + TH + halo - 1 (columns likewise), zeros
 *             outside the field
 *   NTY, NTX  tiles per direction; blocks = NTY NTX K B
 *   rows, pitch  each of the two LDS tables (n and o) holds rows = TH + 2 halo + 1 rows of pitch = TW + 2 halo + 1 ints (row 0 and
 *             column 0 are the zeros of the summed-area table); pitch is odd
 *   lds       bytes of LDS per block: the two tables, the two histograms of S + 1 int32 bins, 4 x 24 int64 of the block reduction
 *   threads   = 256;  ws = 0: no workspace (the raw sums are added across the tiles by 64-bit integer atomics)
 * S, B, H, W >= 1, 1 <= K <= 4, 1 <= NS <= 8 and valid widths, else -1; S > 1024, B > 65535, H W >= 2^31 - 256 or S^2 w_max^4 H W >=
 * 2^63: -2; dims, scales or plan null: -3. */
int tmg_ens_event_plan(const int64_t* dims, const int64_t* scales, int64_t* plan);

/* tmg_ens_event_count runs once per chunk of k whole members: y holds the chunk's rows, [k][B][HW] pixels of C fp32 channels, pixel
 * stride y_d[0], channel offset y_d[1] (tmg_ens_score_store's rule: channel slices of wider buffers work).  Counts into the planar
 * cnt [B][K][HW] int32: the chunk with m0 = 0 writes, later chunks add.  No member buffer is needed.
 * dims = {k, B, HW, C, S, m0, K}.  2 <= C <= 4, 1 <= K <= 4, k >= 1, 0 <= m0, m0 + k <= S, every channel in 0 .. C - 1, every
 * direction 0 or 1, y_d[0] >= y_d[1] + C, else -1; S > 1024 or sizes beyond the index ranges: -2; a null pointer: -3. */
int tmg_ens_event_count(const void* y, const int64_t* y_d, const void* thr, const int64_t* ev, void* cnt, const int64_t* dims,
                        tmg_stream_t st);

/* tmg_ens_event_step runs once per kept step, after the step's last chunk is counted.  target: [B][HW] pixels of C fp32 channels,
 * pixel stride t_d[0], channel offset t_d[1] (normalised, as the members).  It zeroes and then fills the step's planes
 *   rel_count, rel_hit  int32, case b at + b * o_d[0], [K][S + 1]
 *   fss_raw             int64, case b at + b * o_d[1], [K][NS][3] = (A, Bx, Cc)
 * and, when flags & 1, advances the per-pixel running sums tsum [4][B][K][HW] int32 = (sum n, sum o, sum n^2, sum n o), which hold
 * t_before steps (t_before = 0: written, not read).  S^2 (t_before + 1) < 2^31 keeps them in range.
 * dims = {S, B, H, W, C, K, NS, t_before, flags}.  Codes as tmg_ens_event_plan and tmg_ens_event_count, and t_before >= 0, o_d[0] >=
 * K (S + 1), o_d[1] >= 3 K NS, else -1; S^2 (t_before + 1) >= 2^31 with flags & 1: -2; a null pointer (tsum only with flags & 1): -3. */
int tmg_ens_event_step(const void* cnt, const void* target, const int64_t* t_d, const void* thr, const int64_t* ev, const int64_t* scales,
                       void* rel_count, void* rel_hit, void* fss_raw, void* tsum, const int64_t* o_d, const int64_t* dims, tmg_stream_t st);

#endif
