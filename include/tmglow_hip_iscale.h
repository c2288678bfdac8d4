/* Intensity-scale verification of the ensemble's events (tmg_iscale.hip): the raw sums from which the host splits the binary error of
 * every member, and the Brier score of the ensemble, into orthogonal 2-D Haar components of dyadic block size 2, 4, .., 2^L plus the
 * coarse remainder (Casati, Ross & Stephenson 2004; the energy form of Casati 2010).  Integer compares, bit counts and adds only
 * (int32 inside a tile, then one 64-bit integer global atomic per non-zero entry and block): integer sums do not depend on their
 * order, so every output is bitwise reproducible, independent of the chunking, and equal to an int64 reference.  A header of its
 * own: tmglow_hip.h (which defines tmg_stream_t) does not include it.
 *
 * THE DEFINITIONS.  An event k (1 <= K <= 4) is (channel ev[2k], direction ev[2k + 1]: 1 for x > thr, 0 for x < thr, both strict)
 * with the raw threshold thr[b * K + k] (device floats), as in tmglow_hip_event.h.  A value that compares false is in no event: NaN
 * in either direction, +-Inf on the side it cannot be on.  Per case b, event k and pixel p of the H x W field: I_m in {0, 1} the
 * indicator of member m, o the target's, n = sum_m I_m.  The blocks of level l (0 <= l <= L, 1 <= L <= 6) are the 2^l x 2^l squares
 * aligned at pixel (0, 0); the field counts as zero outside H x W, so any H, W >= 1 is accepted and a block cut by the border holds
 * fewer pixels.  s_l(z) is the sum of z over one block of level l.  The raw sums, over all blocks of the level, for l = 0 .. L:
 *   A[m][l] = sum s_l(I_m)^2     X[m][l] = sum s_l(I_m) s_l(o)     Cc[l] = sum s_l(o)^2
 *   AN[l]   = sum s_l(n)^2       XN[l]   = sum s_l(n) s_l(o)
 * No error field is formed: by linearity the block sums of I_m - o give A - 2 X + Cc and those of n - S o give AN - 2 S XN + S^2 Cc.
 *
 * THE LAYOUTS, all of one kept step.
 *   cnt    [B][K][HW] int32           n per pixel: the chunk with m0 = 0 writes it, later chunks add.  No memset: where several
 *                                     blocks share a tile (below) the zeroing launch of the m0 = 0 call covers it.
 *   member [B][K][S][L + 1][2] int64  (A, X) per member and level
 *   target [B][K][L + 1] int64        Cc per level
 *   ens    [B][K][L + 1][2] int64     (AN, XN) per level
 * The chunk call with m0 = 0 zeroes all three tables of the step before its own launch: no memset.
 *
 * THE KERNELS' SHAPE.  One block of 256 threads per 64 x 64 tile of one (case, event) plane.  The chunk kernel loads rows of 64
 * consecutive pixels, one per lane: the lane mask of the compare is a row of the member's indicator, and 64 of them in LDS are the
 * tile.  A thread holds a 4 x 4 patch of it (one 16-bit mask per member) and forms levels 0 - 2 itself; a wave is 8 x 8 patches, 32 x 32 pixels, and forms levels 3 - 5 by lane
 * exchanges at xor distances (1, 8), (2, 16), (4, 32); level 6 combines the four waves through LDS.  Dyadic blocks up to 64 nest
 * in the tiles, which are aligned at pixel (0, 0) as well.  Lanes whose pixels lie outside the field carry zero bits and stay for
 * every exchange and barrier. */
#ifndef TMGLOW_HIP_ISCALE_H
#define TMGLOW_HIP_ISCALE_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_iscale_plan launches nothing: the launch plan of tmg_ens_iscale_chunk and tmg_ens_iscale_step for dims = {S, B, H, W, K,
 * L}, which the launch bodies themselves call.  out (14 host integers) = {tile, tiles_x, tiles_y, grid_x, grid_y, grid_z, blocks,
 * threads, group, lds_bytes, step_lds_bytes, member_words, target_words, ens_words}:
 *   tile                     = 64; tiles_x, tiles_y = ceil(W / 64), ceil(H / 64)
 *   grid_x, grid_y, grid_z   = tiles_x tiles_y, K, B; blocks = their product, of threads = 256.  The step kernel's grid, and the
 *                            chunk kernel's for one member group: it launches grid_y ceil(k / group(k)) blocks in y
 *   group                    = group(S), where group(k), the members one block takes of a chunk of k, is min(k, G) with G the largest
 *                            of 8, 4, 2 for which blocks ceil(k / G) >= 512, else 2: a block forms the target's patch once for its
 *                            members, so larger groups read less and smaller ones fill the chip.  The sums do not depend on it.
 *   lds_bytes, step_lds_bytes  the (static) LDS of the chunk and of the step kernel
 *   member_words, target_words, ens_words = B K S (L + 1) 2, B K (L + 1), B K (L + 1) 2 64-bit words
 * S, B, H, W >= 1, 1 <= K <= 4, 1 <= L <= 6, else -1; S > 1024, B > 65535, H W >= 2^31 - 256 or S^2 4^L H_pad W_pad >= 2^63 (H_pad,
 * W_pad: H, W rounded up to multiples of 64): -2; a null pointer: -3. */
int tmg_ens_iscale_plan(const int64_t* dims, int64_t* out);

/* tmg_ens_iscale_chunk handles one chunk of k whole members plus the step's target: y holds the chunk's rows, [k][B][HW] pixels of C
 * fp32 channels, pixel stride y_d[0], channel offset y_d[1] (tmg_ens_event_count's rule: channel slices of wider buffers work), read
 * straight from the NHWC rows; target: [B][HW] pixels of C channels, pixel stride t_d[0], channel offset t_d[1].  It adds (A, X) of
 * the members m0 .. m0 + k - 1 into member and folds their indicators into cnt (m0 = 0 writes, later chunks add).  The call with
 * m0 = 0 first zeroes member, target and ens and also adds the step's Cc into target.
 * dims = {k, B, H, W, C, S, m0, K, L}.  The plan's limits, 2 <= C <= 4, k >= 1, 0 <= m0, m0 + k <= S, every channel in 0 .. C - 1,
 * every direction 0 or 1, y_d[0] >= y_d[1] + C, y_d[1] >= 0 (t_d alike), else -1; the plan's -2, and y or target beyond the index
 * ranges: -2; a null pointer: -3.  Every code comes before any launch. */
int tmg_ens_iscale_chunk(const void* y, const int64_t* y_d, const void* target, const int64_t* t_d, const void* thr, const int64_t* ev,
                         void* cnt, void* member, void* target_tab, void* ens, const int64_t* dims, tmg_stream_t st);

/* tmg_ens_iscale_step is called once per kept step, after the step's last chunk: it adds (AN, XN), formed from cnt and the target,
 * into ens.
 * dims = {S, B, H, W, C, K, L}: the codes of tmg_ens_iscale_chunk.  Every code comes before any launch. */
int tmg_ens_iscale_step(const void* cnt, const void* target, const int64_t* t_d, const void* thr, const int64_t* ev, void* ens,
                        const int64_t* dims, tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
