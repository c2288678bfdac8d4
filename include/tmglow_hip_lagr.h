/* Lagrangian transport of the ensemble members and of the target (tmg_lagr.hip): pathlines of a lattice of seed particles through
 * every row's own velocity field, then the flow map's finite-time Lyapunov exponent, displacements, residence times and endpoint
 * statistics in fp64.  No atomics, no LDS, no workspace: bitwise reproducible for every chunking.  A header of its own: tmglow_hip.h
 * (which defines tmg_stream_t) does not include it.
 *
 * THE DEFINITIONS (stated once here; the tests' float32 mirror follows them operation by operation).  fl() is one fp32 rounding; no
 * operation is contracted.
 *   rows        the S members plus the target as row S
 *   positions   pixel coordinates: px along W, py along H, pixel (h, w) at (px, py) = (w, h).  A position is INSIDE when
 *               0 <= px <= W - 1 && 0 <= py <= H - 1 (a NaN fails both comparisons: outside)
 *   velocity    pixels per kept step: c_c = fl(fl(a_c y_c) + o_c), c = 0, 1, with the fp32 tables a [B][2], o [B][2]
 *   bilinear    of a plane f at an inside position:  j0 = min((int)floorf(px), W - 2), i0 = min((int)floorf(py), H - 2),
 *               fx = fl(px - j0), fy = fl(py - i0), top = fl(f[i0,j0] + fl(fx fl(f[i0,j0+1] - f[i0,j0]))), bot the same on row
 *               i0 + 1, value = fl(top + fl(fy fl(bot - top)))
 *   in time     V(s) = fl(v0 + fl(s fl(v1 - v0))) with v0 the bilinear value of the previous timed step's plane (prev) and v1 that
 *               of the current one, both at the same position
 *   advection   n = substeps Heun steps, j = 0 .. n - 1, with s_j = float32(j / n), h = float32(1 / n), hh = float32(0.5 / n):
 *               k1 = V(s_j) at x;  x* = fl(x + fl(h k1)), not inside: the particle dies;  k2 = V(s_{j+1}) at x*;
 *               xn = fl(x + fl(hh fl(k1 + k2))), not inside: the particle dies, else x = xn.
 *               A dead particle keeps its last inside position, records the index of the advection that killed it in `exit`
 *               (0 for the first advection; -1 while alive) and is never touched again
 *   seeds       the lattice of pixels (oy + i sy, ox + j sx), i < Gh, j < Gw, P = Gh Gw <= H W particles, particle p = i Gw + j
 *   timed steps the first one (t_before == 0) seeds, counts the residence and stores the planes; every later one runs one
 *               advection, counts the residence of the particles still alive and then overwrites the planes
 *   residence   boxes (h0, h1, w0, w1), inclusive: an alive particle with h0 <= py <= h1 && w0 <= px <= w1 adds 1 to its counter
 * State: pos [S + 1][B][2][P] fp32 (px, then py), exit [S + 1][B][P] int32, res [S + 1][B][R][P] int32, prev [S + 1][B][2][HW] fp32. */
#ifndef TMGLOW_HIP_LAGR_H
#define TMGLOW_HIP_LAGR_H

#include "tmglow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* tmg_ens_lagr_plan launches nothing: the launch plans of tmg_ens_lagr_advect and tmg_ens_lagr_store for dims = {S, B, H, W, P},
 * which the launch bodies themselves call.  plan (6 host integers) = {TILE, NT, STILE, SNT, vec, bytes}:
 *   TILE   particles of one advect block (256 threads, one particle per thread): 256
 *   NT     = ceil(P / TILE); the advect grid is NT x B x k
 *   STILE  pixels of one store block (256 threads): 1024 on the vector path (4 consecutive pixels per thread), else 256
 *   SNT    = ceil(H W / STILE); the store grid is SNT x B x k
 *   vec    1: the planes of prev are written with 16-byte stores, which a call takes when W % 4 == 0 AND the base of prev is 16-byte
 *          aligned; the plan assumes an aligned base, so vec = (W % 4 == 0)
 *   bytes  of pos, exit and prev: (S + 1) B (12 P + 8 H W); res adds 4 R P per row and case
 * S, B >= 1, H, W >= 2, 1 <= P <= H W, else -1; S > 1024, B > 65535 or sizes beyond the index ranges: -2; a null pointer: -3. */
int tmg_ens_lagr_plan(const int64_t* dims, int64_t* plan);

/* tmg_ens_lagr_advect: rows [k B][H W] pixels of fp32 channels (ux, uy first), pixel stride t_d[0], channel offset t_d[1] (raw
 * normalised values; row s B + b is member row0 + s of case b; the target is fed as k = 1, row0 = S).  Device tables a, o [B][2].
 * seeds (24 HOST integers) = {Gh, Gw, oy, ox, sy, sx, R, n, then (h0, h1, w0, w1) of 4 boxes}; hs (11 HOST floats) = {s_0 .. s_8, h,
 * hh}.  With t_before == 0 every particle of the rows is seeded (pos, exit = -1, res = its first count; prev is not read); else
 * the particles with exit < 0 run advection number t_before - 1 as defined above and count their residence.  One thread owns one
 * particle of one row of one case; an element of the state is touched by that thread alone, once per call.  The inside test comes
 * before any index is formed and every gather index is clamped as an integer immediately before its load, so that no input value,
 * non-finite ones included, addresses anything outside the row's field or outside prev.
 * dims = {k, S, B, H, W, row0, t_before}.  Codes as tmg_ens_lagr_plan, and k >= 1, 0 <= row0, row0 + k <= S + 1, t_before >= 0,
 * t_d[0] >= t_d[1] + 2, t_d[1] >= 0, Gh, Gw, sy, sx >= 1, oy, ox >= 0, the lattice inside the field, 0 <= R <= 4, 1 <= n <= 8, every
 * used box inside the field with h0 <= h1, w0 <= w1, else -1. */
int tmg_ens_lagr_advect(const void* rows, const int64_t* t_d, const void* a, const void* o, const void* prev, void* pos, void* exit,
                        void* res, const int64_t* seeds, const float* hs, const int64_t* dims, tmg_stream_t st);

/* tmg_ens_lagr_store: prev[row0 + s][b][c][q] = fl(fl(a_c y_c) + o_c) of the chunk's rows, c = 0, 1.  AFTER tmg_ens_lagr_advect of
 * the same rows, on the same stream: the advection reads the planes this call overwrites.  dims = {k, S, B, H, W, row0}. */
int tmg_ens_lagr_store(const void* rows, const int64_t* t_d, const void* a, const void* o, void* prev, const int64_t* dims,
                       tmg_stream_t st);

/* tmg_ens_lagr_finalize: the state after Tn timed steps; fl (4 HOST doubles) = {dx, dy, step_dt, T_int}, all positive and finite.
 * One thread per case and lattice node, fp64 arithmetic, fp32 outputs; a Welford mean / M2 over the members in member order (n = n +
 * 1, d = v - mean, mean = mean + d / n, M2 = M2 + d (v - mean)) that counts only the members valid at the node; std = sqrt(M2 / n);
 * NaN where n == 0.  Physical positions are (X, Y) = (px dx, py dy); a row is ALIVE at a node when its exit < 0.
 *   FTLE     valid at an interior lattice node whose row is alive there and at its four lattice neighbours:
 *            F11 = (X[i,j+1] - X[i,j-1]) / (2 sx dx), F21 the same of Y, F12 = (X[i+1,j] - X[i-1,j]) / (2 sy dy), F22 the same of Y,
 *            C11 = F11^2 + F21^2, C12 = F11 F12 + F21 F22, C22 = F12^2 + F22^2, hd = (C11 - C22) / 2,
 *            lam = (C11 + C22) / 2 + sqrt(hd^2 + C12^2), ftle = ln(lam) / (2 T_int)
 *   disp     ((px - px0) dx, (py - py0) dy) with (px0, py0) the seed, over the alive members
 *   res_time counter * step_dt, over all members
 *   end_err  the distance sqrt((X_m - X_S)^2 + (Y_m - Y_S)^2) over the members alive together with the target
 *   end_spread  sqrt(var X + var Y) of the alive members' endpoints about their mean (population variances, Welford)
 * outs (17 HOST pointers to device arrays, fp32 unless stated): ftle_mean, ftle_std, target_ftle [B][P], ftle_count [B][P] int32,
 * disp_mean, disp_std, target_disp [B][2][P], alive_frac (alive members / S), target_alive [B][P], res_time_mean, res_time_std,
 * target_res_time [B][R][P] (null when R == 0), end_err_mean, end_spread [B][P], and, all three or none, member_ftle [B][S][P],
 * member_end [B][S][2][P] (pos itself, in pixels), member_exit [B][S][P] int32.  dims = {S, B, H, W}; seeds as above. */
int tmg_ens_lagr_finalize(const void* pos, const void* exit, const void* res, const double* fl, void* const* outs, const int64_t* seeds,
                          const int64_t* dims, tmg_stream_t st);

#ifdef __cplusplus
}
#endif

#endif
