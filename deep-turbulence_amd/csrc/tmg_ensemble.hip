// Ensemble statistics of sampled roll-outs (TMGlow.sampleEnsemble / utils.modelPredStats): the per-step mean and spread over the
// members of every channel and of the velocity magnitude (the plotting scripts' np.std(pred_mag, axis=0), plotCylinderVelocity.py:
// 68-71), and per member the time mean and RMS fluctuation of every channel (target0_mean / target0_rms, trainFlowParallel.py:
// 237-238) with their mean and spread over the members.
//   ens_accum_kernel          one roll-out step of a chunk of k members -> running (mean, M2) of the step (Welford inside the
//                             chunk, Chan's merge with the chunks before) and of every member over time (Welford over the steps);
//                             the step's last chunk writes mean and population std straight into the planar outputs
//   ens_time_finalize_kernel  once at the end: per member time mean and sqrt(M2 / T), then their mean and std over the members
//   ens_turb_accum_kernel     the same chunk's turbulence statistics: vorticity w = dv/dx - du/dy of every member (3x3 stencil of pc/),
//                             its mean / std over the members per step, and per member the time co-moment of (u, v) and the time
//                             mean of w
//   ens_turb_finalize_kernel  once at the end: per member <u'v'>, k = 0.5 (<u'u'> + <v'v'>) and time-mean w, then their mean and std
//                             over the members
// Bandwidth kernels: one thread owns one pixel of one case, every state array is planar ([..][HW], lanes on consecutive pixels),
// so all state traffic is coalesced.  fp32 Welford (no E[y^2] - E[y]^2 cancellation), no atomics: bitwise reproducible.
#include "tmg_field.h"
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
                std_out[o] = sqrtf(tmg_relu(m2[c]) * rn);
            }
        }
        mag_mean[(size_t)b * mcs + p] = mean[ENS_MAXC];
        mag_std[(size_t)b * mcs + p] = sqrtf(tmg_relu(m2[ENS_MAXC]) * rn);
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
            const float rv = sqrtf(tmg_relu(tm2[i]) * rT);
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
        tm_std[e] = sqrtf(tmg_relu(aq) * rs);
        rms_mean[e] = rm;
        rms_std[e] = sqrtf(tmg_relu(rq) * rs);
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

// Turbulence statistics of the chunk ens_accum_kernel folds: launched BEFORE ens_accum_kernel on the same chunk, because the time
// co-moment C_uv += (u - mean_u_old) (v - mean_v_new) reads the members' running time means of channels 0 and 1 from ens_accum_kernel's
// tmean planes as they stand before that kernel advances them (no planes of its own for them: two loads per member and step instead
// of two loads and two stores); mean_v_new is formed here by the same Welford step.  tmean is read-only here, so ens_accum_kernel's
// results do not depend on whether this kernel ran.
// Stencil operands: direct neighbour loads, no LDS tile.  A thread needs u at (h +- 1, w - 1 .. w + 1) and v at (h - 1 .. h + 1, w +- 1);
// the neighbours along W are the adjacent lanes' own pixels (same cache lines), the rows above and below are lines the neighbouring
// waves load anyway, and one member's two channels of a 256 x 256 case (<= 1.1 MB at pixel stride 4) stay in L1 / L2 between the three
// row passes.  The input is NHWC with a run-time pixel stride, so an LDS tile would be filled by the same strided loads and save
// only the re-reads the caches already serve, at the price of a barrier per member; the kernel stays bound by its state planes.
// One thread per pixel of a case, state planar, no atomics: bitwise reproducible.  The physical values are tmg_unnorm_fma's, which
// are ens_accum_kernel's yh bit for bit.
__global__ __launch_bounds__(256) void ens_turb_accum_kernel(const float* __restrict__ y, int ps, const float* __restrict__ u,
                                                             const float* __restrict__ out_mu, const float* __restrict__ out_std,
                                                             const float* __restrict__ tmean, float* __restrict__ vmean,
                                                             float* __restrict__ vm2, float* __restrict__ cuv, float* __restrict__ tvort,
                                                             float* __restrict__ vort_mean, float* __restrict__ vort_std, long long vcs,
                                                             int k, int B, int Hh, int Ww, int C, int n_before, int m0, int t_before,
                                                             int flags, float rdx, float rdy) {
    const int HW = Hh * Ww;
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (p >= HW) return;
    const int h = p / Ww, w = p - h * Ww;
    const float sc0 = u ? u[b * C] : 1.f, sc1 = u ? u[b * C + 1] : 1.f;
    const float mu0 = out_mu[0], mu1 = out_mu[1], sd0 = out_std[0], sd1 = out_std[1];
    const bool up = h > 0, dn = h + 1 < Hh, lf = w > 0, rt = w + 1 < Ww;   // zero padding: a neighbour outside the field is 0
    const size_t hw = (size_t)HW;
    const long long rs = (long long)Ww * ps;         // one row down
    float mean = 0.f, m2 = 0.f;                      // this chunk's Welford state of the vorticity
    const float tn = 1.f / (float)(t_before + 1);
    for (int j = 0; j < k; ++j) {
        const float* yp = y + ((size_t)(j * B + b) * hw + p) * ps;
        // d/dx v: columns w +- 1 of rows h - 1, h, h + 1 weighted 1, 2, 1; d/dy u: rows h +- 1 of columns w - 1, w, w + 1 weighted 1, 2, 1
        const float vx = tmg_sx<true>(yp, ps, rs, 1, sc1, sd1, mu1, up, dn, lf, rt);
        const float uy = tmg_sy<true>(yp, ps, rs, 0, sc0, sd0, mu0, up, dn, lf, rt);
        const float vort = vx * rdx - uy * rdy;      // rdx = 1 / (8 dx), rdy = 1 / (8 dy)
        const float rn = 1.f / (float)(j + 1);
        const float d = vort - mean;
        mean += d * rn;
        m2 += d * (vort - mean);
        if (flags & 1) {                             // the member's time statistics: one more step
            const size_t ti = ((size_t)(m0 + j) * B + b) * hw + p;
            float cq = 0.f, tw = 0.f, du = 0.f, dv = 0.f;   // first step: mean_v_new = v, the co-moment starts at 0
            if (t_before > 0) {
                const size_t tb = ((size_t)(m0 + j) * B + b) * C * hw + p;   // channel 0 of the member's tmean planes
                const float uu = tmg_unnorm_fma(yp[0], sc0, sd0, mu0), vv = tmg_unnorm_fma(yp[1], sc1, sd1, mu1);
                const float mv_old = tmean[tb + hw];
                du = uu - tmean[tb];
                dv = vv - (mv_old + (vv - mv_old) * tn);   // v - mean_v_new
                cq = cuv[ti];
                tw = tvort[ti];
            }
            cuv[ti] = cq + du * dv;
            tvort[ti] = tw + (vort - tw) * tn;
        }
    }
    // Chan's merge with the n_before members of the step's earlier chunks
    const size_t si = (size_t)b * hw + p;
    const float n = (float)(n_before + k);
    if (n_before > 0) {
        const float fa = (float)n_before, fb = (float)k;
        const float ma = vmean[si], qa = vm2[si];
        const float d = mean - ma;
        mean = ma + d * (fb / n);
        m2 = qa + m2 + d * d * (fa * fb / n);
    }
    if (flags & 2) {
        vort_mean[(size_t)b * vcs + p] = mean;
        vort_std[(size_t)b * vcs + p] = sqrtf(tmg_relu(m2) * (1.f / n));
    } else {
        vmean[si] = mean;
        vm2[si] = m2;
    }
}

extern "C" int tmg_ens_turb_accum(const void* y, const int64_t* y_d, const void* u, const void* out_mu, const void* out_std,
                                  const void* tmean, void* vmean, void* vm2, void* cuv, void* tvort, void* vort_mean, void* vort_std,
                                  const int64_t* dims, const float* fl, hipStream_t st) {
    const int64_t k = dims[0], B = dims[1], Hh = dims[2], Ww = dims[3], C = dims[4], n_before = dims[5], m0 = dims[6],
                  t_before = dims[7], flags = dims[8], vcs = dims[9];
    if (k < 1 || B < 1 || Hh < 1 || Ww < 1 || C < 2 || C > ENS_MAXC || n_before < 0 || m0 < 0 || t_before < 0) return -1;
    if (y_d[0] < C || y_d[1] < 0 || y_d[1] + C > y_d[0]) return -1;
    if (!(fl[0] > 0.f) || !(fl[1] > 0.f) || !(fl[0] <= 3.0e38f) || !(fl[1] <= 3.0e38f)) return -1;
    if (Hh >= (1ll << 31) || Ww >= (1ll << 31)) return -2;
    const int64_t HW = Hh * Ww;
    if ((flags & 2) && vcs < HW) return -1;
    if ((k * B) * HW * y_d[0] >= (1ll << 40) || k * B > (1ll << 30) || HW >= (1ll << 31) - 256 || B > 65535) return -2;
    if (!y || !out_mu || !out_std) return -3;
    if (!(flags & 2) && (!vmean || !vm2)) return -3;
    if ((flags & 2) && (!vort_mean || !vort_std)) return -3;
    if (n_before > 0 && (!vmean || !vm2)) return -3;
    if ((flags & 1) && (!cuv || !tvort || (t_before > 0 && !tmean))) return -3;
    dim3 grid((unsigned)((HW + 255) / 256), (unsigned)B);
    hipLaunchKernelGGL(ens_turb_accum_kernel, grid, dim3(256), 0, st, (const float*)y + y_d[1], (int)y_d[0], (const float*)u,
                       (const float*)out_mu, (const float*)out_std, (const float*)tmean, (float*)vmean, (float*)vm2, (float*)cuv,
                       (float*)tvort, (float*)vort_mean, (float*)vort_std, (long long)vcs, (int)k, (int)B, (int)Hh, (int)Ww, (int)C,
                       (int)n_before, (int)m0, (int)t_before, (int)flags, 0.125f / fl[0], 0.125f / fl[1]);
    TMG_CHECK_LAUNCH();
    return 0;
}

// One thread per (case, pixel) element e of [B][HW]; member m's co-moment and time-mean vorticity at m * B*HW + e, its M2 of
// channels 0 and 1 (ens_accum_kernel's tm2 planes) at ((m * B + b) * C + c) * HW + p.
__global__ __launch_bounds__(256) void ens_turb_finalize_kernel(const float* __restrict__ tm2, const float* __restrict__ cuv,
                                                                const float* __restrict__ tvort, float* __restrict__ uv_mean,
                                                                float* __restrict__ uv_std, float* __restrict__ tke_mean,
                                                                float* __restrict__ tke_std, float* __restrict__ tv_mean,
                                                                float* __restrict__ tv_std, int S, int B, int HW, int C, float rT) {
    const size_t n = (size_t)B * HW;
    for (size_t e = blockIdx.x * (size_t)256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const size_t b = e / HW, p = e - b * HW;
        float am[3] = {0.f, 0.f, 0.f}, aq[3] = {0.f, 0.f, 0.f};   // Welford over the members of <u'v'>, k, time-mean w
        for (int m = 0; m < S; ++m) {
            const size_t i = (size_t)m * n + e;
            const size_t i2 = (((size_t)m * B + b) * C) * HW + p;
            float v[3];
            {
                // rounded products: fused into v - mean below, the first member would leave M2 = rounding error instead of 0
#pragma clang fp contract(off)
                v[0] = cuv[i] * rT;
                v[1] = 0.5f * (tm2[i2] + tm2[i2 + HW]) * rT;
                v[2] = tvort[i];
            }
            const float rn = 1.f / (float)(m + 1);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float d = v[q] - am[q];
                am[q] += d * rn;
                aq[q] += d * (v[q] - am[q]);
            }
        }
        const float rs = 1.f / (float)S;
        uv_mean[e] = am[0];
        uv_std[e] = sqrtf(tmg_relu(aq[0]) * rs);
        tke_mean[e] = am[1];
        tke_std[e] = sqrtf(tmg_relu(aq[1]) * rs);
        tv_mean[e] = am[2];
        tv_std[e] = sqrtf(tmg_relu(aq[2]) * rs);
    }
}

extern "C" int tmg_ens_turb_finalize(const void* tm2, const void* cuv, const void* tvort, void* uv_mean, void* uv_std, void* tke_mean,
                                     void* tke_std, void* tv_mean, void* tv_std, const int64_t* dims, hipStream_t st) {
    const int64_t S = dims[0], B = dims[1], HW = dims[2], C = dims[3], T = dims[4];
    if (S < 1 || B < 1 || HW < 1 || C < 2 || C > ENS_MAXC || T < 1) return -1;
    if (HW >= (1ll << 31) || B >= (1ll << 31) || S >= (1ll << 31) || B * HW >= (1ll << 40)) return -2;
    if (!tm2 || !cuv || !tvort || !uv_mean || !uv_std || !tke_mean || !tke_std || !tv_mean || !tv_std) return -3;
    size_t g = ((size_t)B * HW + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(ens_turb_finalize_kernel, dim3((unsigned)g), dim3(256), 0, st, (const float*)tm2, (const float*)cuv,
                       (const float*)tvort, (float*)uv_mean, (float*)uv_std, (float*)tke_mean, (float*)tke_std, (float*)tv_mean,
                       (float*)tv_std, (int)S, (int)B, (int)HW, (int)C, 1.f / (float)T);
    TMG_CHECK_LAUNCH();
    return 0;
}
