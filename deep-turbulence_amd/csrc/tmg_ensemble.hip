// Ensemble statistics of sampled roll-outs (TMGlow.sampleEnsemble / utils.modelPredStats): the per-step mean and spread over the
// members of every channel and of the velocity magnitude (the plotting scripts' np.std(pred_mag, axis=0), plotCylinderVelocity.py:
// 68-71), and per member the time mean and RMS fluctuation of every channel (target0_mean / target0_rms, trainFlowParallel.py:
// 237-238) with their mean and spread over the members.
//   ens_accum_kernel          one roll-out step of a chunk of k members -> running (mean, M2) of the step (Welford inside the
//                             chunk, Chan's merge with the chunks before) and of every member over time (Welford over the steps);
//                             the step's last chunk writes mean and population std straight into the planar outputs
//   ens_time_finalize_kernel  once at the end: per member time mean and sqrt(M2 / T), then their mean and std over the members
// Bandwidth kernels: one thread owns one pixel of one case, every state array is planar ([..][HW], lanes on consecutive pixels),
// so all state traffic is coalesced.  fp32 Welford (no E[y^2] - E[y]^2 cancellation), no atomics: bitwise reproducible.
#include "tmg_common.h"
#include "tmglow_hip.h"

#define ENS_MAXC 4

__global__ __launch_bounds__(256) void ens_accum_kernel(const float* __restrict__ y, int ps, const float* __restrict__ u,
                                                        const float* __restrict__ out_mu, const float* __restrict__ out_std,
                                                        float* __restrict__ smean, float* __restrict__ sm2, float* __restrict__ tmean,
                                                        float* __restrict__ tm2, float* __restrict__ mean_out, float* __restrict__ std_out,
                                                        float* __restrict__ mag_mean, float* __restrict__ mag_std, long long ocs,
                                                        long long mcs, int k, int B, int HW, int C, int n_before, int m0, int t_before,
                                                        int flags) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= HW) return;
    float sc[ENS_MAXC], mu[ENS_MAXC], sd[ENS_MAXC];
#pragma unroll
    for (int c = 0; c < ENS_MAXC; ++c) {
        sc[c] = (c < C && u) ? u[b * C + c] : 1.f;
        mu[c] = c < C ? out_mu[c] : 0.f;
        sd[c] = c < C ? out_std[c] : 0.f;
    }
    const size_t hw = (size_t)HW;
    float mean[ENS_MAXC + 1], m2[ENS_MAXC + 1];     // this chunk's Welford state: channels 0..C-1, then |u| (index ENS_MAXC)
#pragma unroll
    for (int c = 0; c <= ENS_MAXC; ++c) mean[c] = m2[c] = 0.f;
    const float tn = 1.f / (float)(t_before + 1);
    for (int j = 0; j < k; ++j) {
        const float* yp = y + ((size_t)(j * B + b) * hw + p) * ps;
        float v[ENS_MAXC + 1];
#pragma unroll
        for (int c = 0; c < ENS_MAXC; ++c) v[c] = c < C ? sc[c] * (sd[c] * yp[c] + mu[c]) : 0.f;
        v[ENS_MAXC] = sqrtf(v[0] * v[0] + v[1] * v[1]);
        const float rn = 1.f / (float)(j + 1);
#pragma unroll
        for (int c = 0; c <= ENS_MAXC; ++c) {
            if (c < C || c == ENS_MAXC) {
                const float d = v[c] - mean[c];
                mean[c] += d * rn;
                m2[c] += d * (v[c] - mean[c]);
            }
        }
        if (flags & 1) {                             // the member's time statistics: one more step
            const size_t tb = ((size_t)(m0 + j) * B + b) * C * hw + p;
#pragma unroll
            for (int c = 0; c < ENS_MAXC; ++c) {
                if (c < C) {
                    const size_t i = tb + (size_t)c * hw;
                    float tmv = 0.f, tmq = 0.f;
                    if (t_before > 0) {
                        tmv = tmean[i];
                        tmq = tm2[i];
                    }
                    const float d = v[c] - tmv;
                    tmv += d * tn;
                    tmq += d * (v[c] - tmv);
                    tmean[i] = tmv;
                    tm2[i] = tmq;
                }
            }
        }
    }
    // Chan's merge with the n_before members of the step's earlier chunks
    const size_t sb = (size_t)b * (C + 1) * hw + p;
    const float n = (float)(n_before + k);
    if (n_before > 0) {
        const float fa = (float)n_before, fb = (float)k;
#pragma unroll
        for (int c = 0; c <= ENS_MAXC; ++c) {
            if (c < C || c == ENS_MAXC) {
                const size_t i = sb + (size_t)(c < C ? c : C) * hw;
                const float ma = smean[i], qa = sm2[i];
                const float d = mean[c] - ma;
                mean[c] = ma + d * (fb / n);
                m2[c] = qa + m2[c] + d * d * (fa * fb / n);
            }
        }
    }
    if (flags & 2) {
        const float rn = 1.f / n;
#pragma unroll
        for (int c = 0; c < ENS_MAXC; ++c) {
            if (c < C) {
                const size_t o = (size_t)b * ocs + (size_t)c * hw + p;
                mean_out[o] = mean[c];
                std_out[o] = sqrtf(fmaxf(m2[c], 0.f) * rn);
            }
        }
        mag_mean[(size_t)b * mcs + p] = mean[ENS_MAXC];
        mag_std[(size_t)b * mcs + p] = sqrtf(fmaxf(m2[ENS_MAXC], 0.f) * rn);
    } else {
#pragma unroll
        for (int c = 0; c <= ENS_MAXC; ++c) {
            if (c < C || c == ENS_MAXC) {
                const size_t i = sb + (size_t)(c < C ? c : C) * hw;
                smean[i] = mean[c];
                sm2[i] = m2[c];
            }
        }
    }
}

extern "C" int tmg_ens_accum(const void* y, const int64_t* y_d, const void* u, const void* out_mu, const void* out_std, void* smean,
                             void* sm2, void* tmean, void* tm2, void* mean_out, void* std_out, void* mag_mean, void* mag_std,
                             const int64_t* o_d, const int64_t* dims, hipStream_t st) {
    const int64_t k = dims[0], B = dims[1], HW = dims[2], C = dims[3], n_before = dims[4], m0 = dims[5], t_before = dims[6],
                  flags = dims[7];
    if (k < 1 || B < 1 || HW < 1 || C < 2 || C > ENS_MAXC || n_before < 0 || m0 < 0 || t_before < 0) return -1;
    if (y_d[0] < C || y_d[1] < 0 || y_d[1] + C > y_d[0]) return -1;
    if ((k * B) * HW * y_d[0] >= (1ll << 40) || k * B > (1ll << 30) || HW >= (1ll << 31) - 256 || B > 65535) return -2;
    if (!(flags & 2) && (!smean || !sm2)) return -3;
    if ((flags & 2) && (!mean_out || !std_out || !mag_mean || !mag_std)) return -3;
    if (n_before > 0 && (!smean || !sm2)) return -3;
    if ((flags & 1) && (!tmean || !tm2)) return -3;
    dim3 grid((unsigned)((HW + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(ens_accum_kernel, grid, dim3(256), 0, st, (const float*)y + y_d[1], (int)y_d[0], (const float*)u,
                       (const float*)out_mu, (const float*)out_std, (float*)smean, (float*)sm2, (float*)tmean, (float*)tm2,
                       (float*)mean_out, (float*)std_out, (float*)mag_mean, (float*)mag_std, (long long)o_d[0], (long long)o_d[1], (int)k,
                       (int)B, (int)HW, (int)C, (int)n_before, (int)m0, (int)t_before, (int)flags);
    TMG_CHECK_LAUNCH();
    return 0;
}

// One thread per (case, channel, pixel) element e of [B][C][HW]; member m's state at m * B*C*HW + e.
__global__ __launch_bounds__(256) void ens_time_finalize_kernel(const float* __restrict__ tmean, const float* __restrict__ tm2,
                                                                float* __restrict__ tm_mean, float* __restrict__ tm_std,
                                                                float* __restrict__ rms_mean, float* __restrict__ rms_std, int S,
                                                                size_t n, float rT) {
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        float am = 0.f, aq = 0.f, rm = 0.f, rq = 0.f;
        for (int m = 0; m < S; ++m) {
            const size_t i = (size_t)m * n + e;
            const float tv = tmean[i];
            const float rv = sqrtf(fmaxf(tm2[i], 0.f) * rT);
            const float rn = 1.f / (float)(m + 1);
            float d = tv - am;
            am += d * rn;
            aq += d * (tv - am);
            d = rv - rm;
            rm += d * rn;
            rq += d * (rv - rm);
        }
        const float rs = 1.f / (float)S;
        tm_mean[e] = am;
        tm_std[e] = sqrtf(fmaxf(aq, 0.f) * rs);
        rms_mean[e] = rm;
        rms_std[e] = sqrtf(fmaxf(rq, 0.f) * rs);
    }
}

extern "C" int tmg_ens_time_finalize(const void* tmean, const void* tm2, void* tm_mean, void* tm_std, void* rms_mean, void* rms_std,
                                     const int64_t* dims, hipStream_t st) {
    const int64_t S = dims[0], B = dims[1], HW = dims[2], C = dims[3], T = dims[4];
    if (S < 1 || B < 1 || HW < 1 || C < 1 || T < 1) return -1;
    const size_t n = (size_t)B * C * HW;
    size_t g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(ens_time_finalize_kernel, dim3((unsigned)g), dim3(256), 0, st, (const float*)tmean, (const float*)tm2,
                       (float*)tm_mean, (float*)tm_std, (float*)rms_mean, (float*)rms_std, (int)S, n, 1.f / (float)T);
    TMG_CHECK_LAUNCH();
    return 0;
}
