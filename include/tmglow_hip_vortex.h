/* Vortex census of the ensemble members and of the target (tmg_vortex.hip): classify every pixel by the Okubo-Weiss criterion and
 * the sign of its vorticity, label the 4-connected components, measure them in int64 and keep a table of them per row, case and
 * timed step.  Integer sums only, no float atomics: every output is bitwise reproducible and independent of the chunking.  A header
 * of its own: tmglow_hip.h (which defines tmg_stream_t) does not include it.
 *
 * THE DEFINITIONS (stated once here; the tests' float32 mirror follows them operation by operation).  fl() is one fp32 rounding; no
 * operation is contracted.
 *   rows        the S members plus the target as row S
 *   physical    of channel c (0: u, 1: v) at a pixel: fl(sc_c fl(fl(sd_c y_c) + mu_c)), sc = u[b][c] (1 without u); outside the field 0
 *   stencils    the un-scaled 3x3 ones of pc/, with the summation order of tmglow_hip_pdf.h: Sx right column first, then left, each
 *               centre * 2, up, down; Sy lower row first, then upper, each centre * 2, left, right
 *   gradients   ux = fl(Sx(u) rdx), uy = fl(Sy(u) rdy), vx = fl(Sx(v) rdx), vy = fl(Sy(v) rdy), rdx = fl(0.125f / fl(dx)), rdy alike
 *   vorticity   w = fl(vx - uy) (bit for bit the `vort` of tmg_pdf.hip), strains sn = fl(ux - vy), ss = fl(vx + uy)
 *   criterion   ow = fl(fl(fl(w w) - fl(sn sn)) - fl(ss ss)): minus the Okubo-Weiss parameter, four times the 2-D Q
 *   fixed point qf = fl(w qscale[b]), qscale[b] a power of two; q = (int64) rint(qf) (ties to even)
 *   class       sign(w) (+1 / -1) when the pixel is not on the one-pixel frame of the field AND ow > thr[b] AND |qf| <= 2^31 AND
 *               q != 0; else 0.  A NaN fails every comparison: non-finite input becomes background
 *   rejected    counts the interior pixels whose ow is NaN, or whose ow > thr[b] while |qf| <= 2^31 fails
 *   component   a maximal 4-connected set of pixels of one non-zero class (opposite signs never merge, diagonals do not connect);
 *               its label is the smallest linear index h W + w in it; background -1
 *   measures    8 int64 words: root, n, sum w, sum h, sum q, sum q w, sum q h, max |q| (w, h: the pixel's column and row)
 *   table       per row, case and timed step: the components with n >= min_area in increasing root order, the first K of them; an
 *               empty slot is {-1, 0, 0, 0, 0, 0, 0, 0}.  found[2] (+, -) counts all of them before the truncation
 *   occupancy   core[b][sign][p] (+: 0, -: 1) counts the pixels of components with n >= min_area, truncated or not
 * State: table [Tk][S + 1][B][K][8] int64, found [Tk][S + 1][B][2] int32, rejected [Tk][S + 1][B] int32, core [2][B][2][HW] int32
 * (members, then the target; zeroed once), status int32 (zeroed once). */
#ifndef TMGLOW_HIP_VORTEX_H
#define TMGLOW_HIP_VORTEX_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_vortex_plan launches nothing: the launch plans for dims = {k, S, B, H, W, K, Tn}, which the launch bodies themselves call.
 * plan (12 host integers) = {TH, TW, NTH, NTW, tile_blocks, merge_blocks, pixel_blocks, threads, lds_label, lds_census, ws_bytes,
 * state_bytes}:
 *   TH, TW        the tile of one labelling block (32 x 32, 256 threads, 4 pixels per thread); NTH = ceil(H / TH), NTW alike
 *   tile_blocks   = NTH NTW per plane: the tile kernel's grid is tile_blocks x (k B)
 *   merge_blocks  = ceil(((NTW - 1) H + (NTH - 1) W) / threads) per plane: one thread per pixel pair across a tile border (0: none)
 *   pixel_blocks  = ceil(H W / threads) per plane: classify, root replacement, areas
 *   lds_label     5 TH TW bytes (parents int32, classes int8); lds_census = max(64 K, 4 * 1024 + 16) (the table slice / the scan)
 *   ws_bytes      17 k B H W: vorticity fp32, labels int32, areas int32, slots int32, classes int8, in that order
 *   state_bytes   64 K (S + 1) B Tn for the tables plus 16 B H W for the two occupancies
 * k, S, B, K, Tn >= 1, H, W >= 3, K <= 256, k <= S + 1, else -1; S > 1024, H or W > 512, k B > 65535: -2; a null pointer: -3. */
int tmg_ens_vortex_plan(const int64_t* dims, int64_t* plan);

/* tmg_ens_vortex_classify: rows [k B][H W] pixels of fp32 channels (u, v first), pixel stride t_d[0], channel offset t_d[1] (raw
 * normalised values, row s B + b is case b).  Device tables u [B][C] (or null), mu [C], sd [C], thr [B], qscale [B] fp32; fl (2 HOST
 * floats) = {dx, dy}.  Writes omega [k B][HW] fp32 and cls [k B][HW] int8 and sets rejected [k B] int32 (zeroed by the call, then
 * counted).  dims = {k, B, H, W, C}; 2 <= C <= 4, t_d[0] >= t_d[1] + C, t_d[1] >= 0, dx, dy positive and finite, else -1. */
int tmg_ens_vortex_classify(const void* rows, const int64_t* t_d, const void* u, const void* mu, const void* sd, const void* thr,
                            const void* qscale, void* omega, void* cls, void* rejected, const float* fl, const int64_t* dims,
                            tmg_stream_t st);

/* tmg_ens_vortex_label: cls [n][HW] int8 -> label [n][HW] int32 as defined above, for any H, W >= 1 (dims = {n, H, W}; n <= 65535,
 * H, W <= 512).  Three launches: every tile is labelled in LDS by a union-find whose links are LDS atomicMin and written as global
 * pixel indices; the pixel pairs of one class across tile borders are united with agent-scope atomic loads and atomicMin on the label
 * plane; every label is replaced by its root.  Kernel boundaries are the only ordering between blocks.  Every loop is bounded by
 * H W + 1 trips; a loop that reaches its bound stores a non-zero code into *status (int32, device, never cleared here):
 * 1 / 2 the tile's find / union, 3 / 4 the merge's, 5 the root replacement. */
int tmg_ens_vortex_label(const void* cls, void* label, void* status, const int64_t* dims, tmg_stream_t st);

/* tmg_ens_vortex_census: label, cls, omega [k B][HW] -> table [k B][K][8] int64, found [k B][2] int32 (both overwritten), and
 * core [B][2][HW] int32 (added to).  area, slot [k B][HW] int32 are workspace (area is zeroed by the call).  Four launches: the
 * areas of the roots (integer atomicAdd); per plane one block that scans the flags "root with area >= min_area" into slots, writes
 * found and the roots of the table and zeroes its other words; per slice of 1024 pixels one block that sums the measures of its
 * pixels in an LDS table and adds the non-zero words to the table (64-bit integer atomics) and 1 to core per pixel of a qualifying
 * component.  dims = {k, B, H, W, K, min_area}; min_area >= 1. */
int tmg_ens_vortex_census(const void* label, const void* cls, const void* omega, const void* qscale, void* area, void* slot,
                          void* table, void* found, void* core, const int64_t* dims, tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
