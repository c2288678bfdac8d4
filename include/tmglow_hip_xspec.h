/* Spectral skill of the ensemble members against the target (tmg_xspec.hip): per wavenumber shell the power, the co-spectrum with
 * the target and the error power of every member and of the ensemble-mean field.  No atomics; every sum has a fixed order, so every
 * output is bitwise reproducible and independent of the chunking.  A header of its own: tmglow_hip.h (which defines tmg_stream_t)
 * does not include it.
 *
 * THE DEFINITIONS.  Rows are the members m = 0 .. S-1, the target T and the ensemble-mean field bar.  Per case b:
 *   f_c = u[b,c] * fmaf(out_std[c], y_c, out_mu[c]) - M[b,c]   c = 0, 1; M: the centre plane [B][2][H][W] (fp32, physical units),
 *                                                              one separate rounding; M null: nothing is subtracted
 *   fbar = (sum_m f_m) / S                                     the members added in member order, one fp32 division
 *   z = g (f_0 + i f_1), Z = fft2(z)                           g: the window folded into the operand matrices of tmg_spec_rows /
 *                                                              the column pass (tmglow_hip.h), the dense DFT on the fp32 matrix pipe
 *   P = sc (zr zr + zi zi), X = sc (zr tr + zi ti), D = sc (dr dr + di di)
 *                                                              sc = 0.5 / (H W)^2; (tr, ti): the target's coefficient of the same
 *                                                              mode; dr = zr - tr, di = zi - ti; every operation rounded on its own
 * and their sums over the shells of a host-built shell map: each 16-column tile's modes in the order of its shell list (perm, offs
 * as tmg_spec_cols takes them), the tiles in tile order.  The shells are symmetric under k -> -k, so the shell sum of X is the
 * vector co-spectrum Re sum(conj(U_m) U_T + conj(V_m) V_T); the quadrature part is not computed.
 * Non-finite members are not supported: the outputs of an affected step are unspecified; no address depends on the data. */
#ifndef TMGLOW_HIP_XSPEC_H
#define TMGLOW_HIP_XSPEC_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_xspec_plan launches nothing: the grids, LDS bytes and buffer sizes of a chunk of k members for dims = {k, B, H, W, NK}.
 * out (11 host integers) = {prep_grid, cols_grid_x, cols_grid_y, cols_lds_bytes, accum_grid_x, accum_grid_y, threads, f_floats,
 * part_floats, zt_floats, part_t_floats}:
 *   prep_grid      = ceil(2 B H W / 256): one thread per element of [B][H][W][2], which loops over the chunk's members
 *   cols grid      = (W / 16, k B): a block owns 16 columns of one image; cols_lds_bytes = 256 H (Y panel and Z tile, [2][H][16] each)
 *   accum grid     = (ceil(NK / 256), 3 B): one thread per (case, quantity of (P, X, D), shell)
 *   f_floats       = 2 k B H W: the dense field buffer f [k B][H][W][2], and the row pass's planar workspace [2][k B][H][W]
 *   part_floats    = 3 k B (W / 16) NK: the cross mode's partial sums [k B][W / 16][3][NK]
 *   zt_floats      = 2 B H W: the target's Z planes [2][B][H][W], and fsum [B][H][W][2]
 *   part_t_floats  = B (W / 16) NK: the target mode's partial sums
 * k, B, NK >= 1, H and W multiples of 16 in [16, 512], else -1; k > 1024, 3 B or k B > 65535, NK > 8192: -2; a null pointer: -3. */
int tmg_ens_xspec_plan(const int64_t* dims, int64_t* out);

/* tmg_ens_xspec_prep forms f of the k images per case of the NHWC chunk y (y_d = {pixel stride, channel offset}: dense rows and
 * channel-slice views of C = 2 .. 4 channels, of which 0 and 1 are read) into f [k B][H][W][2].  dims = {k, B, H, W, C, mode, S,
 * f_floats}.  mode 0: f alone (the target, k = 1); 1: the step's first chunk of members, fsum [B][H][W][2] is stored (no memset);
 * 2: a later chunk, fsum is loaded, added to in member order and stored; 3: f [B][H][W][2] = fsum / S (k = 1; y, u, the tables and
 * center are not read).  u [B][2] or null (1), out_mu / out_std [2], center [B][2][H][W] or null.
 * Codes: the plan's; a mode outside 0 .. 3, S < 1, C outside 2 .. 4, a descriptor that does not hold C channels, mode 3 with
 * k != 1: -1; S > 1024 or a chunk beyond the index range: -2; a null pointer that the mode reads or writes: -3; f_floats under the
 * plan's: -4.  Every code comes before any launch. */
int tmg_ens_xspec_prep(const void* y, const int64_t* y_d, const void* u, const void* out_mu, const void* out_std, const void* center,
                       void* f, void* fsum, const int64_t* dims, tmg_stream_t st);

/* tmg_ens_xspec_cols is the column transform Z = F_H Y of the n images of the row pass's workspace yw [2][n][H][W] (ft [2][H][H]:
 * the operand matrix of tmg_spec_cols; the same product, lane for lane) and the shell sums of every 16-column tile.
 * dims = {n, B, H, W, NK, cross, yw_floats, zt_floats, part_floats}, fl = {sc}.
 *   cross = 0 (n = B, the target): Z goes planar into zt [2][B][H][W], part [B][W / 16][NK] = the sums of P
 *   cross = 1 (n = k B, rows member-major): zt is read, image i against case i mod B; part [n][W / 16][3][NK] = the sums of (P, X, D)
 * Codes: shape limits of the plan, n no multiple of B, cross = 0 with n != B, sc not in (0, 3e38]: -1; n > 65535 or NK > 8192: -2;
 * a null pointer: -3; a buffer under its size: -4. */
int tmg_ens_xspec_cols(const void* ft, const void* yw, const void* perm, const void* offs, void* zt, void* part, const int64_t* dims,
                       const float* fl, tmg_stream_t st);

/* tmg_ens_xspec_accum folds one chunk: per (case, quantity, shell) the tiles' partial sums in tile order, then
 *   the chunk's members in member order into the step sums step [B][3][NK] (n_before = 0: they start at 0) and, flags & 1, into
 *     tmem [B][S][3][NK], each member's sums over the timed steps in step order (t_before = 0: stored, not added);
 *   n_before = 0: the target's P from part_t into tpow [B][Tk][NK] at step t and, flags & 1, into ttgt [B][NK];
 *   flags & 2, the step's last chunk: the mean field's (P, X, D) from part_b [B][W / 16][3][NK] into bar_out [B][Tk][3][NK] at step t
 *     and, flags & 1, into tbar [B][3][NK]; the step sums into sum_out [B][Tk][3][NK] at step t instead of step.
 * dims = {k, B, NK, QT, S, Tk, t, n_before, m0, t_before, flags}.  Codes: a size under 1, QT > 32, t outside 0 .. Tk - 1, flags
 * outside 0 .. 3, m0 != n_before, m0 + k > S, or flags & 2 set on a chunk that is not the last (or clear on the last): -1; sizes
 * beyond the limits of the plan or the index range: -2; a null pointer among those the flags make it touch: -3. */
int tmg_ens_xspec_accum(const void* part, const void* part_t, const void* part_b, void* step, void* tpow, void* sum_out, void* bar_out,
                        void* tmem, void* ttgt, void* tbar, const int64_t* dims, tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
