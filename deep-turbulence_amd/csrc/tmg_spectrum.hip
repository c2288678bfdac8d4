// Shell-binned kinetic-energy spectra E(k) of sampled roll-outs (tmg_ops.EnsembleSpectrum / utils.modelPredSpectra): per member and
// kept step the 2-D DFT of z = g (u + i v) (g: separable window, folded into the operand matrices), E2 = 0.5 |Z|^2 / (HW)^2 summed
// over the shells of a host-built bin map, then mean / population std over the members per step and of each member's time mean.
//   spec_rows_kernel      row transform Y = z F_W^T on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32): a block owns 16 rows of one image,
//                         un-normalises channels 0 and 1 of the NHWC chunk into LDS once (run-time pixel stride, as ens_accum_kernel) and
//                         its four waves share out the 16-mode column tiles; Y goes planar (re, im) into the caller's workspace
//   spec_cols_kernel      column transform Z = F_H Y: a block owns 16 columns of one image (the Y panel in LDS), its waves share out the
//                         16-mode row tiles; the epilogue forms E2 into an LDS tile and sums it per shell in the fixed order of a
//                         host-built list (the tile's modes sorted by shell) -> one partial spectrum per (image, column tile)
//   spec_accum_kernel     one thread per (case, shell): the partial spectra of a member summed in tile order, Welford over the chunk's
//                         members, Chan's merge with the chunks before, per member the running time mean (flags as ens_accum_kernel)
//   spec_finalize_kernel  once at the end: mean and population std over the members of their time means
// The operand matrices, the MFMA lane maps, the side limit and the column pass's product: tmg_dft.h.
// No atomics anywhere (an LDS float atomic from four waves lands in arrival order): the same inputs give the same bits.
#include "tmg_dft.h"
#include "tmg_field.h"
#include "tmglow_hip.h"

#define SPEC_MAXNK 8192

__global__ __launch_bounds__(256) void spec_rows_kernel(const float* __restrict__ y, int ps, const float* __restrict__ u,
                                                        const float* __restrict__ out_mu, const float* __restrict__ out_std,
                                                        const float* __restrict__ ft, float* __restrict__ yw, size_t plane, int B, int Hh,
                                                        int Ww) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    // row stride = 4 (mod 16): the 16 rows x 4 columns of an A fragment fall into 64 different banks
    const int LS = Ww + 4;
    const int img = blockIdx.y, y0 = blockIdx.x * 16;
    const int b = img % B;
    const float sc0 = u ? u[b * 2] : 1.f, sc1 = u ? u[b * 2 + 1] : 1.f;
    const float mu0 = out_mu[0], mu1 = out_mu[1], sd0 = out_std[0], sd1 = out_std[1];
    const float* yp = y + ((size_t)img * Hh + y0) * Ww * ps;
    for (int i = threadIdx.x; i < 16 * Ww; i += 256) {
        const int r = i / Ww, x = i - r * Ww;
        const float* q = yp + (size_t)i * ps;
        lds[r * LS + x] = tmg_unnorm_fma(q[0], sc0, sd0, mu0);
        lds[(16 + r) * LS + x] = tmg_unnorm_fma(q[1], sc1, sd1, mu1);
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, l16 = l & 15, lq = l >> 4;
    const float* au = lds + l16 * LS + lq;
    const float* av = au + 16 * LS;
    const size_t tw = (size_t)Ww * Ww;
    for (int qt = wave; qt < (Ww >> 4); qt += 4) {
        const float* fr = ft + (size_t)lq * Ww + qt * 16 + l16;
        const float* fi = fr + tw;
        f32x4 re = {0.f, 0.f, 0.f, 0.f}, im = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Ww; k0 += 16)        // W is a multiple of 16
#pragma unroll
        for (int k = k0; k < k0 + 16; k += 4) {
            const float a_u = au[k], a_v = av[k];
            const float b_r = fr[(size_t)k * Ww], b_i = fi[(size_t)k * Ww];
            // (u + i v) (b_r + i b_i)
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(a_u, b_r, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(a_u, b_i, im, 0, 0, 0);
            re = __builtin_amdgcn_mfma_f32_16x16x4f32(a_v, -b_i, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_16x16x4f32(a_v, b_r, im, 0, 0, 0);
        }
        float* o = yw + ((size_t)img * Hh + y0 + lq * 4) * Ww + qt * 16 + l16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            o[(size_t)r * Ww] = re[r];
            o[plane + (size_t)r * Ww] = im[r];
        }
    }
}

extern "C" int tmg_spec_rows(const void* y, const int64_t* y_d, const void* u, const void* out_mu, const void* out_std, const void* ft,
                             void* yw, const int64_t* dims, hipStream_t st) {
    const int64_t k = dims[0], B = dims[1], Hh = dims[2], Ww = dims[3], C = dims[4], yw_floats = dims[5];
    if (k < 1 || B < 1 || C < 2 || C > 4) return -1;
    if (!tmg_dft_side_ok(Hh) || !tmg_dft_side_ok(Ww)) return -1;
    if (y_d[0] < C || y_d[1] < 0 || y_d[1] + C > y_d[0]) return -1;
    if (k * B > 65535 || (k * B) * Hh * Ww * y_d[0] >= (1ll << 40)) return -2;
    if (!y || !out_mu || !out_std || !ft || !yw) return -3;
    const int64_t plane = k * B * Hh * Ww;
    if (yw_floats < 2 * plane) return -4;
    const size_t smem = (size_t)2 * 16 * (Ww + 4) * sizeof(float);
    TMG_LDS_OPTIN(spec_rows_kernel);
    hipLaunchKernelGGL(spec_rows_kernel, dim3((unsigned)(Hh / 16), (unsigned)(k * B)), dim3(256), smem, st, (const float*)y + y_d[1],
                       (int)y_d[0], (const float*)u, (const float*)out_mu, (const float*)out_std, (const float*)ft, (float*)yw,
                       (size_t)plane, (int)B, (int)Hh, (int)Ww);
    TMG_CHECK_LAUNCH();
    return 0;
}

// LDS: the Y panel [2][H][16] (re, im), the E2 tile [H][16], the tile's shell sums [NK].
__global__ __launch_bounds__(256) void spec_cols_kernel(const float* __restrict__ ft, const float* __restrict__ yw, size_t plane,
                                                        const int* __restrict__ perm, const int* __restrict__ offs,
                                                        float* __restrict__ part, int Hh, int Ww, int NK, float scale) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int img = blockIdx.y, qt = blockIdx.x, QT = gridDim.x;
    const int HP = Hh * 16;
    float* e2 = lds + 2 * HP;
    float* sums = lds + 3 * HP;
    const float* ysrc = yw + (size_t)img * Hh * Ww + qt * 16;
    for (int i = threadIdx.x; i < HP; i += 256) {
        const size_t g = (size_t)(i >> 4) * Ww + (i & 15);
        lds[i] = ysrc[g];
        lds[HP + i] = ysrc[plane + g];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, l16 = l & 15, lq = l >> 4;
    const float* br = lds + lq * 16 + l16;
    const float* bi = br + HP;
    const size_t th = (size_t)Hh * Hh;
    for (int pt = wave; pt < (Hh >> 4); pt += 4) {
        const float* fr = ft + (size_t)lq * Hh + pt * 16 + l16;
        const float* fi = fr + th;
        f32x4 zr = {0.f, 0.f, 0.f, 0.f}, zi = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < Hh; k0 += 16)        // H is a multiple of 16; the column product of tmg_dft.h
#pragma unroll
        for (int k = k0; k < k0 + 16; k += 4) {
            const float a_r = fr[(size_t)k * Hh], a_i = fi[(size_t)k * Hh];
            const float b_r = br[k * 16], b_i = bi[k * 16];
            zr = __builtin_amdgcn_mfma_f32_16x16x4f32(a_r, b_r, zr, 0, 0, 0);
            zi = __builtin_amdgcn_mfma_f32_16x16x4f32(a_r, b_i, zi, 0, 0, 0);
            zr = __builtin_amdgcn_mfma_f32_16x16x4f32(-a_i, b_i, zr, 0, 0, 0);
            zi = __builtin_amdgcn_mfma_f32_16x16x4f32(a_i, b_r, zi, 0, 0, 0);
        }
        float* e = e2 + (pt * 16 + lq * 4) * 16 + l16;
#pragma unroll
        for (int r = 0; r < 4; ++r) e[r * 16] = scale * (zr[r] * zr[r] + zi[r] * zi[r]);
    }
    __syncthreads();
    // shell sums of the tile in list order: positions of[s] .. of[s + 1] - 1 of pm hold the tile indices (p * 16 + column) of shell s
    const int* pm = perm + (size_t)qt * HP;
    const int* of = offs + (size_t)qt * (NK + 1);
    for (int s = threadIdx.x; s < NK; s += 256) {
        float a = 0.f;
        const int i1 = of[s + 1];
        for (int i = of[s]; i < i1; ++i) a += e2[pm[i]];
        sums[s] = a;
    }
    __syncthreads();
    float* o = part + ((size_t)img * QT + qt) * NK;
    for (int s = threadIdx.x; s < NK; s += 256) o[s] = sums[s];     // store-only
}

extern "C" int tmg_spec_cols(const void* ft, const void* yw, const void* perm, const void* offs, void* part, const int64_t* dims,
                             const float* fl, hipStream_t st) {
    const int64_t n = dims[0], Hh = dims[1], Ww = dims[2], NK = dims[3], yw_floats = dims[4], part_floats = dims[5];
    if (n < 1 || NK < 1) return -1;
    if (!tmg_dft_side_ok(Hh) || !tmg_dft_side_ok(Ww)) return -1;
    if (!(fl[0] > 0.f) || !(fl[0] <= 3.0e38f)) return -1;
    if (n > 65535 || NK > SPEC_MAXNK) return -2;
    if (!ft || !yw || !perm || !offs || !part) return -3;
    const int64_t plane = n * Hh * Ww, QT = Ww / 16;
    if (yw_floats < 2 * plane || part_floats < n * QT * NK) return -4;
    const size_t smem = ((size_t)3 * Hh * 16 + NK) * sizeof(float);
    TMG_LDS_OPTIN(spec_cols_kernel);
    hipLaunchKernelGGL(spec_cols_kernel, dim3((unsigned)QT, (unsigned)n), dim3(256), smem, st, (const float*)ft, (const float*)yw,
                       (size_t)plane, (const int*)perm, (const int*)offs, (float*)part, (int)Hh, (int)Ww, (int)NK, fl[0]);
    TMG_CHECK_LAUNCH();
    return 0;
}

__global__ __launch_bounds__(256) void spec_accum_kernel(const float* __restrict__ part, float* __restrict__ smean,
                                                         float* __restrict__ sm2, float* __restrict__ tmean,
                                                         float* __restrict__ mean_out, float* __restrict__ std_out, long long ocs, int k,
                                                         int B, int NK, int QT, int n_before, int m0, int t_before, int flags) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (s >= NK) return;
    float mean = 0.f, m2 = 0.f;                      // this chunk's Welford state of E[s]
    const float tn = 1.f / (float)(t_before + 1);
    for (int j = 0; j < k; ++j) {
        const float* pp = part + (size_t)(j * B + b) * QT * NK + s;
        float E = 0.f;
        for (int t = 0; t < QT; ++t) E += pp[(size_t)t * NK];      // the column tiles' partial spectra in tile order
        const float rn = 1.f / (float)(j + 1);
        const float d = E - mean;
        mean += d * rn;
        m2 += d * (E - mean);
        if (flags & 1) {                             // the member's running time mean: one more step
            const size_t ti = ((size_t)(m0 + j) * B + b) * NK + s;
            const float tm = t_before > 0 ? tmean[ti] : 0.f;
            tmean[ti] = tm + (E - tm) * tn;
        }
    }
    // Chan's merge with the n_before members of the step's earlier chunks
    const size_t si = (size_t)b * NK + s;
    const float n = (float)(n_before + k);
    if (n_before > 0) {
        const float fa = (float)n_before, fb = (float)k;
        const float ma = smean[si], qa = sm2[si];
        const float d = mean - ma;
        mean = ma + d * (fb / n);
        m2 = qa + m2 + d * d * (fa * fb / n);
    }
    if (flags & 2) {
        mean_out[(size_t)b * ocs + s] = mean;
        std_out[(size_t)b * ocs + s] = sqrtf(fmaxf(m2, 0.f) * (1.f / n));
    } else {
        smean[si] = mean;
        sm2[si] = m2;
    }
}

extern "C" int tmg_spec_accum(const void* part, void* smean, void* sm2, void* tmean, void* mean_out, void* std_out, const int64_t* dims,
                              hipStream_t st) {
    const int64_t k = dims[0], B = dims[1], NK = dims[2], QT = dims[3], n_before = dims[4], m0 = dims[5], t_before = dims[6],
                  flags = dims[7], ocs = dims[8];
    if (k < 1 || B < 1 || NK < 1 || QT < 1 || QT > TMG_DFT_MAXN / 16 || n_before < 0 || m0 < 0 || t_before < 0) return -1;
    if ((flags & 2) && ocs < NK) return -1;
    if (k * B > 65535 || B > 65535 || NK > SPEC_MAXNK || m0 + k > (1ll << 30)) return -2;
    if (!part) return -3;
    if (!(flags & 2) && (!smean || !sm2)) return -3;
    if ((flags & 2) && (!mean_out || !std_out)) return -3;
    if (n_before > 0 && (!smean || !sm2)) return -3;
    if ((flags & 1) && !tmean) return -3;
    hipLaunchKernelGGL(spec_accum_kernel, dim3((unsigned)((NK + 255) / 256), (unsigned)B), dim3(256), 0, st, (const float*)part,
                       (float*)smean, (float*)sm2, (float*)tmean, (float*)mean_out, (float*)std_out, (long long)ocs, (int)k, (int)B,
                       (int)NK, (int)QT, (int)n_before, (int)m0, (int)t_before, (int)flags);
    TMG_CHECK_LAUNCH();
    return 0;
}

// One thread per (case, shell) element e of [B][NK]; member m's time mean at m * B*NK + e.
__global__ __launch_bounds__(256) void spec_finalize_kernel(const float* __restrict__ tmean, float* __restrict__ tm_mean,
                                                            float* __restrict__ tm_std, int S, int n) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float am = 0.f, aq = 0.f;
    for (int m = 0; m < S; ++m) {
        const float tv = tmean[(size_t)m * n + e];
        const float d = tv - am;
        am += d * (1.f / (float)(m + 1));
        aq += d * (tv - am);
    }
    tm_mean[e] = am;
    tm_std[e] = sqrtf(fmaxf(aq, 0.f) * (1.f / (float)S));
}

extern "C" int tmg_spec_finalize(const void* tmean, void* tm_mean, void* tm_std, const int64_t* dims, hipStream_t st) {
    const int64_t S = dims[0], B = dims[1], NK = dims[2];
    if (S < 1 || B < 1 || NK < 1) return -1;
    if (S >= (1ll << 30) || B > 65535 || NK > SPEC_MAXNK) return -2;
    if (!tmean || !tm_mean || !tm_std) return -3;
    const int64_t n = B * NK;
    hipLaunchKernelGGL(spec_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)tmean, (float*)tm_mean,
                       (float*)tm_std, (int)S, (int)n);
    TMG_CHECK_LAUNCH();
    return 0;
}
