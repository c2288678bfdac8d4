/* Launch-plan queries of libtmglow_hip.so's convolution launchers, direct and Winograd, and of the growth-layer forwards and the thin / mix weight gradients.  Included by tmglow_hip.h (which defines tmg_stream_t): do not
 * include it on its own.  The operations are declared in tmglow_hip.h; these entry points compute nothing. */
#ifndef TMGLOW_HIP_PLAN_H
#define TMGLOW_HIP_PLAN_H

/* Launch-plan queries of the three launchers above: the arguments of the launch plus `plan`; nothing is launched, no pointer is
 * dereferenced and no device is needed (without one the planners assume 256 compute units); the return value is the code the launch
 * would return.  The launchers themselves fill `plan`, immediately before the point where they would launch.
 *   tmg_conv_fwd_plan: plan[16] = {kernel (0 conv_fwd_kernel, 1 conv_mfma_kernel), MT, NTW, WM, WN, TW_log2, TH, tiles_x, tiles_y, KCH,
 *     nchunks, grid_x, grid_y, lds_bytes, vec4, ovec4}
 *   tmg_conv_wgrad_plan (ngroups > 1: the plan of tmg_conv_wgrad_grouped): plan[15] = {NP, NCO, LEAN, ksplit, MPIX, TH, TW_log2, CITG,
 *     PPG, gx, gy, gz, slab path (ws accepted), lds_bytes, ws_floats}
 *   tmg_conv_rep_border_plan: plan[5] = {mfma (0 scalar kernel, 1 matrix-core kernel), NT, ksplit S, 16-pixel tiles, blocks} */
int tmg_conv_fwd_plan(const void* const* in_ptrs, const int64_t* in_desc, int64_t nseg, const void* wpk, const void* bias,
                      const void* kappa, const void* in_scale, const void* in_shift, const void* add, const int64_t* add_desc,
                      void* const* out_ptrs, const int64_t* out_desc, int64_t nout, const int64_t* dims, tmg_stream_t st,
                      int64_t* plan);
int tmg_conv_wgrad_plan(const void* const* in_ptrs, const int64_t* in_desc, int64_t nseg, const void* in_scale,
                        const void* in_shift, const void* dy, const int64_t* dy_desc, void* dW, void* dbias, const void* kappa,
                        void* ws, int64_t ws_floats, const int64_t* dims, tmg_stream_t st, int64_t ngroups, int64_t* plan);
int tmg_conv_rep_border_plan(const void* dy, const int64_t* dy_desc, const void* w, const void* kappa, void* const* out_ptrs,
                             const int64_t* out_desc, int64_t nout, const int64_t* dims, tmg_stream_t st, int64_t* plan);

/* The same for the Winograd launchers (tmg_wino.hip):
 *   tmg_conv_wino_fwd_plan, tmg_conv_wino_fwd3_plan, tmg_conv_wino_narrow_plan: plan[13] = {kernel (0 wino_fwd_kernel, 1 wino_fwdp_kernel,
 *     2 wino_fwd3_kernel, 3 wino_nn_kernel), NPW (wino_nn_kernel: NTN), Cin_pad, nchunks, 16-channel groups of the last 32-channel chunk,
 *     Npad / 16, tiles_x, tiles_y, ntiles, grid_x, grid_y, largest tile count of one block, lds_bytes}
 *   tmg_conv_wino_wgrad_plan (ngroups > 1: the plan of tmg_conv_wino_wgrad_grouped): plan[11] = {CIT, NCO, DB (two tile buffers), gx, gy,
 *     gz, bpg (block rows per group), NG of wino_wgrad_reduce_kernel, ntiles, lds_bytes, ws_floats} */
int tmg_conv_wino_fwd_plan(const void* const* in_ptrs, const int64_t* in_desc, int64_t nseg, const void* U, const void* bias,
                           void* const* out_ptrs, const int64_t* out_desc, int64_t nout, const int64_t* dims, tmg_stream_t st,
                           int64_t* plan);
int tmg_conv_wino_fwd3_plan(const void* const* in_ptrs, const int64_t* in_desc, int64_t nseg, const void* U, const void* bias,
                            void* const* out_ptrs, const int64_t* out_desc, int64_t nout, const int64_t* dims, tmg_stream_t st,
                            int64_t* plan);
int tmg_conv_wino_narrow_plan(const void* const* in_ptrs, const int64_t* in_desc, int64_t nseg, const void* U, const void* bias,
                              void* const* out_ptrs, const int64_t* out_desc, int64_t nout, const int64_t* dims, tmg_stream_t st,
                              int64_t* plan);
int tmg_conv_wino_wgrad_plan(const void* const* in_ptrs, const int64_t* in_desc, int64_t nseg, const void* dy, const int64_t* dy_desc,
                             void* dW, void* dbias, void* ws, int64_t ws_floats, const int64_t* dims, tmg_stream_t st, int64_t ngroups,
                             int64_t* plan);

/* The same for the growth-layer forwards (tmg_pointwise.hip) and the thin / mix weight gradients (tmg_thin.hip):
 *   tmg_c1x2_fwd_plan: plan[12] = {CG (threads per pixel), TW_log2, TH, tiles_x, tiles_y, t256 (256-pixel tiles, which select CG), KCH,
 *     nchunks, nring (ring pixels of a tile's d1 region), grid, lds_bytes, vec4}
 *   tmg_c1_fwd_plan (the plan of tmg_c1_fwd_add): plan[9] = {TW_log2, TH, tiles_x, tiles_y, KCH, nchunks, grid, lds_bytes, vec4}
 *   tmg_conv_wgrad_thin_grouped_plan: plan[11] = {SL, CS, TH, dyc, tiles_x, tiles_y, ntiles, P, xcd (P % 8 == 0: the XCD-aware block
 *     order), grid, lds_bytes}
 *   tmg_mix_wgrad_grouped_plan: plan[5] = {CT, U, P, per (pixels per partition), grid} */
int tmg_c1x2_fwd_plan(const void* const* in_ptrs, const int64_t* in_desc, int64_t nseg, const void* w1, const void* w2, const void* add1,
                      const int64_t* add1_d, const void* add2, const int64_t* add2_d, void* out, const int64_t* out_d, const int64_t* dims,
                      tmg_stream_t st, int64_t* plan);
int tmg_c1_fwd_plan(const void* const* in_ptrs, const int64_t* in_desc, int64_t nseg, const void* w, const void* add,
                    const int64_t* add_d, void* out, const int64_t* out_d, const int64_t* dims, tmg_stream_t st, int64_t* plan);
int tmg_conv_wgrad_thin_grouped_plan(const void* gtab, int64_t G, const int64_t* seg_channels, int64_t nseg, const void* dy,
                                     int64_t dy_stride, void* dW, const int64_t* dims, tmg_stream_t st, int64_t* plan);
int tmg_mix_wgrad_grouped_plan(const void* gtab, int64_t G, void* dW, void* db, const int64_t* dims, tmg_stream_t st, int64_t* plan);

#endif
