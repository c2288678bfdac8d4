/* Layout conversions of the level node's backward pass (tmg_thin.hip).  Included by tmglow_hip.h (which defines tmg_stream_t): do not
 * include it on its own. */
#ifndef TMGLOW_HIP_LAYOUT_H
#define TMGLOW_HIP_LAYOUT_H

/* The inverse of tmg_layer_planes: K float2 planes [K][npix][2] (the per-layer (dd1, dd2) gradients of the growth channels, which
 * tmg_dense2_bwd writes plane-wise on large levels and tmg_conv_wgrad_thin_grouped reads one plane per group) -> [npix][CP] with
 * channel 2k / 2k+1 = plane k and the channels from 2 K on zero: the layout the level-wide conditioning contractions read.
 * 1 <= K <= CP / 2, CP a multiple of 4, 4 <= CP <= 512 (64 (CP + 2) floats of LDS); -1 otherwise, nothing launched. */
int tmg_layer_unplanes(const void* src, void* dst, int64_t npix, int64_t CP, int64_t K, tmg_stream_t st);

#endif
