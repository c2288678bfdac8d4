/* Probability densities of the flow quantities pooled over regions of the flow, for the ensemble members and for the target
 * (tmg_pdf.hip: marginal and joint histograms; integer adds only, no float atomics: bitwise reproducible and independent of the
 * chunking).  Included by tmglow_hip.h (which defines tmg_stream_t): do not include it on its own.
 *
 * Fields.  There are up to 8, each one of: a channel 0..C-1 (aliases "ux", "uy", "p" for 0, 1, 2), "speed", "vort", "div".  The three
 * derived fields need grid = (dx, dy).  (The launcher's kind codes: 0..3 a channel, 4 speed, 5 vort, 6 div.)
 * Values for a channel field.  The value binned is d = x, the raw normalised value: u out_std > 0 keeps the order, and comparisons
 * have no rounding.  With an optional centre it is one rounded fp32 subtraction, d = fl(x - c_raw[b, c, p]).
 * Values for a derived field.  The physical value is formed in fp32 with every operation rounded on its own (contraction off, no
 * fused multiply-add, so that a numpy float32 mirror reproduces it exactly):
 *   t = fl(fl(sd x) + mu), then v = fl(u t).
 *   The 3x3 first-derivative stencil of pc/ is applied with zero padding: a neighbour outside the field is 0 in physical units, with
 *   exactly the neighbours, weights and summation order of ens_turb_accum_kernel: right column first, then left, each in the order
 *   centre * 2, up, down (d/dx); lower row first, then upper, each in the order centre * 2, left, right (d/dy).
 *   rdx = fl(0.125f / fl(dx)), rdy = fl(0.125f / fl(dy)).
 *   vort = fl(fl(vx rdx) - fl(uy rdy)), vx = d/dx of channel 1, uy = d/dy of channel 0.
 *   div = fl(fl(ux_x rdx) + fl(vy_y rdy)), with the same stencil transposed: ux_x = d/dx of channel 0, vy_y = d/dy of channel 1.
 *   speed = sqrt_rn(fl(fl(U U) + fl(V V))), with a correctly rounded square root.
 * Edges.  Each field has nb uniform inner bins, 1 <= nb <= 128, the same nb for all fields.  The physical edges are
 * E_j = lo + j (hi - lo) / nb, j = 0..nb, formed in fp64.  The device table e[b][f][j] is fp32, formed in fp64 and rounded once:
 *   channel field without centre: (E_j / u[b,c] - mu[c]) / sd[c]
 *   channel field with centre:    E_j / (u[b,c] sd[c]), with c_raw = float32((center / u - mu) / sd)
 *   derived field:                E_j itself
 * Edges that are not strictly increasing after rounding are a ValueError.  (tmg_ops.pdf_edge_tables raises it; the launcher takes the
 * tables as given.)
 * Bin index.  Defined by comparisons alone: idx(d) = #{ j in 0..nb : d >= e_j }.  So 0 is the underflow bin (d < e_0), nb + 1 is
 * the overflow bin (d >= e_nb), and a value ON an edge belongs to the bin above it.  Non-finite members are not supported.
 * Regions.  There are up to 4 pixel boxes (x0, x1, y0, y1), half open, x along W.  They may overlap.  Each must be non-empty and
 * inside the field.  A pixel is counted in every region that holds it.  A derived field at a region's border still uses its
 * neighbours outside the region.  Only the field border pads with zeros.
 * Joint histograms.  There are up to 2 pairs (fi, fj) of distinct listed fields.  Each axis has nbj uniform bins, 1 <= nbj <= 32,
 * over the same [lo, hi] as its field, with its own rounded edge table je[b][pair][axis][nbj + 1] and the same index rule.  The
 * table is (nbj + 2)^2 counts and fi indexes its rows. */
#ifndef TMGLOW_HIP_PDF_H
#define TMGLOW_HIP_PDF_H

/* tmg_ens_pdf_plan launches nothing: the launch plan of tmg_ens_pdf_count for dims = {k, B, H, W, F, nb, P, nbj, R, derived}
 * (derived: 1 when a field is speed, vort or div), which the launch body itself calls.  plan (8 host integers) =
 * {SL, NSL, lds, copies, instance, threads, blocks, PPT}:
 *   SL, NSL   one block takes the pixels [s SL, min(HW, (s + 1) SL)) of one row (member, case), NSL slices per row; SL = 256 PPT,
 *             PPT = 4 pixels per thread (thread t: pixels t, t + 256, ..)
 *   lds       bytes of LDS per block: the edge tables and one guess scale per table (F + 2 P floats), `copies` marginal
 *             histograms [R][F][nb + 2], the joint histograms [R][P][(nbj + 2)^2], all int32 / fp32
 *   copies    the number of private marginal histograms: 1 (equal indices of a wave are aggregated before the LDS add)
 *   instance  0: channel fields only; 1: with derived fields (neighbour loads, un-normalisation)
 *   threads   = 256;  blocks = NSL k B
 * k, B, H, W, F, R >= 1, F <= 8, R <= 4, 1 <= nb <= 128, 0 <= P <= 2, 1 <= nbj <= 32 (P > 0), else -1; k B > 65535 or H W >= 2^31 -
 * 1024: -2; dims or plan null: -3. */
int tmg_ens_pdf_plan(const int64_t* dims, int64_t* plan);

/* tmg_ens_pdf_count runs once per chunk of k whole members (the target: a chunk of one member into planes of its own).  y holds the
 * chunk's rows, [k][B][H W] pixels of C fp32 channels, pixel stride y_d[0], channel offset y_d[1].  u [B][C] (null: 1), mu, sd [C]
 * (device floats; read with derived fields only).  center: c_raw [B][C][H W] or null.  edges [B][F][nb + 1], jedges
 * [B][P][2][nbj + 1] (device floats).  desc (host integers) = F kinds, then P x (fi, fj), then R x (x0, x1, y0, y1).  fl = {dx, dy}
 * (host floats; read with derived fields only).  It ADDS into (the caller zeroes them)
 *   step_count  int32, case b at + b * o_d[0], [R][F][nb + 2]: this step's plane, pooled over members and pixels
 *   step_joint  int32, case b at + b * o_d[1], [R][P][(nbj + 2)^2]                                      (P > 0)
 * and, when flags & 1 (a timed step), into
 *   member_time_count [B][S][R][F][nb + 2] int32 (member m0 + j of the chunk), time_joint [B][R][P][(nbj + 2)^2] int32.
 * dims = {k, B, H, W, C, S, m0, F, nb, P, nbj, R, flags}.  Sizes as tmg_ens_pdf_plan, 2 <= C <= 4, 0 <= m0, m0 + k <= S, kinds in
 * 0..C-1 or 4..6, pairs of distinct fields below F, boxes non-empty and inside the field, o_d not smaller than the planes, positive
 * finite dx, dy with derived fields, else -1; sizes beyond the index ranges: -2; a null pointer that is needed: -3. */
int tmg_ens_pdf_count(const void* y, const int64_t* y_d, const void* u, const void* mu, const void* sd, const void* center,
                      const void* edges, const void* jedges, const int64_t* desc, void* step_count, void* step_joint,
                      void* member_time_count, void* time_joint, const int64_t* o_d, const int64_t* dims, const float* fl,
                      tmg_stream_t st);

#endif
