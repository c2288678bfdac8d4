// Temporal power spectra of sampled roll-outs (tmg_ops.EnsembleTimeSpectrum / utils.modelPredTimeSpectra): per element e of
// [S][B][C][HW] (member, case, channel, pixel; E of them) the one-sided power spectral density over the Tn fed steps of the
// un-normalised series xh_n = u[b][c] (out_std[c] y_n + out_mu[c]):
//   xbar = mean_n xh_n,  d_n = g_n (xh_n - xbar),  X_k = sum_n d_n exp(-2 pi i k n / Tn),  P_k = c_k |X_k|^2 / Tn^2,  k = 0 .. NF - 1
// (g: the periodic Hann window over its RMS, or 1; c_k = 1 at k = 0 and at the Nyquist bin of an even Tn, else 2), then the mean and
// population std of P_k over the members.  Updating 2 NF accumulator planes at every step would move 8 NF bytes per element and step
// against 4 bytes of input, so the transform is blocked in time:
//   tspec_store_kernel     one chunk of k members, NHWC -> un-normalised rows m0 .. m0 + k - 1 of slot (step mod 16) of the planar
//                          ring [16][E] (ens_score_store_kernel's transpose plus the affine)
//   tspec_block_kernel     after every 16th step, and once for the remainder: acc[r][e] (+)= sum_j tm[n0 + j][r] ring[j][e] on the
//                          fp32 matrix pipe (v_mfma_f32_16x16x4_f32, K = the block's steps).  Rows r of acc [R][E], R = 2 NF + 1:
//                          re_k = sum g_n cos at row k, im_k = sum -g_n sin at row NF + k, the plain sum of xh (for xbar) at row 2 NF.
//                          A wave owns 64 consecutive elements (four 16-column tiles, the ring fragment read once) and walks the
//                          16-row tiles; the first block writes acc, later blocks add.  The ring comes from torch.empty: slots >= nb
//                          are not read and their MFMAs are not issued (0 * NaN is NaN).
//   tspec_finalize_kernel  one thread per (case, bin, channel, pixel): per member X_k = (re_k, im_k) - xbar G_k with the host-built
//                          G_k = sum_n g_n exp(-2 pi i k n / Tn), P_k = (c_k / Tn^2) |X_k|^2, Welford over the members in order
// The operand tm [Tn][RP] (RP = R rounded up to 16, the padding columns zero) is built on the host in fp64 with the argument reduced
// in integers, (k n) mod Tn, and rounded once.  MFMA lane maps (16x16x4 f32, as tmg_dft.h): A[i = l & 15][k = l >> 4],
// B[k = l >> 4][j = l & 15], C/D column l & 15, rows 4 (l >> 4) + 0..3: the D columns are consecutive elements (pixels), so every
// accumulator row is read and written in 64-byte runs.  An MFMA is a k-ordered fmaf chain onto its C input: acc after a block is the
// chain over the block's steps in order, started from acc before it.
// No atomics anywhere: the same inputs give the same bits.
#include "tmg_dft.h"
#include "tmg_field.h"
#include "tmglow_hip.h"

#define TSPEC_MAXC 4
#define TSPEC_RING 16

__global__ __launch_bounds__(256) void tspec_store_kernel(const float* __restrict__ y, int ps, const float* __restrict__ u,
                                                          const float* __restrict__ out_mu, const float* __restrict__ out_std,
                                                          float* __restrict__ ring, int B, int HW, int C, int m0) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y, j = blockIdx.z;
    if (p >= HW) return;
    const size_t hw = (size_t)HW;
    const float* yp = y + ((size_t)(j * B + b) * hw + p) * ps;
    float* xp = ring + ((size_t)(m0 + j) * B + b) * C * hw + p;
#pragma unroll
    for (int c = 0; c < TSPEC_MAXC; ++c)
        if (c < C) {
            const float sc = u ? u[b * C + c] : 1.f;
            xp[(size_t)c * hw] = tmg_unnorm_fma(yp[c], sc, out_std[c], out_mu[c]);
        }
}

extern "C" int tmg_tspec_store(const void* y, const int64_t* y_d, const void* u, const void* out_mu, const void* out_std, void* ring,
                               const int64_t* dims, hipStream_t st) {
    const int64_t k = dims[0], B = dims[1], HW = dims[2], C = dims[3], S = dims[4], m0 = dims[5], slot = dims[6];
    if (k < 1 || B < 1 || HW < 1 || C < 2 || C > TSPEC_MAXC || S < 1 || m0 < 0 || m0 + k > S || slot < 0 || slot >= TSPEC_RING) return -1;
    if (y_d[0] < C || y_d[1] < 0 || y_d[1] + C > y_d[0]) return -1;
    if (HW >= (1ll << 31) - 256 || B > 65535 || k > 65535 || y_d[0] >= (1ll << 31) || S >= (1ll << 30)) return -2;
    if ((k * B) * HW * y_d[0] >= (1ll << 40) || S * B * C * HW >= (1ll << 40)) return -2;
    if (!y || !out_mu || !out_std || !ring) return -3;
    const int64_t E = S * B * C * HW;
    dim3 grid((unsigned)((HW + 255) / 256), (unsigned)B, (unsigned)k);
    hipLaunchKernelGGL(tspec_store_kernel, grid, dim3(256), 0, st, (const float*)y + y_d[1], (int)y_d[0], (const float*)u,
                       (const float*)out_mu, (const float*)out_std, (float*)ring + slot * E, (int)B, (int)HW, (int)C, (int)m0);
    TMG_CHECK_LAUNCH();
    return 0;
}

__global__ __launch_bounds__(256) void tspec_block_kernel(const float* __restrict__ tm, const float* __restrict__ ring,
                                                          float* __restrict__ acc, size_t E, int R, int RP, int n0, int nb, int first) {
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, l16 = l & 15, lq = l >> 4;
    const size_t e0 = ((size_t)blockIdx.x * 4 + wave) * 64 + l16;           // this lane's element of column tile 0
    if (e0 - l16 >= E) return;                                             // the whole wave is beyond the end
    // B fragments of the wave's four column tiles: bv[q][ct] = ring[4 q + lq][e0 + 16 ct], zero where there is nothing valid
    float bv[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = 4 * q + lq;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const size_t e = e0 + 16 * ct;
            bv[q][ct] = (j < nb && e < E) ? ring[(size_t)j * E + e] : 0.f;
        }
    }
    for (int r0 = 0; r0 < RP; r0 += 16) {
        float av[4];                                                       // A fragments: av[q] = tm[n0 + 4 q + lq][r0 + l16]
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = 4 * q + lq;
            av[q] = j < nb ? tm[(size_t)(n0 + j) * RP + r0 + l16] : 0.f;
        }
        const int rr = r0 + 4 * lq;                                        // this lane's first D row
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const size_t e = e0 + 16 * ct;
            float* ap = acc + (size_t)rr * E + e;
            f32x4 d = {0.f, 0.f, 0.f, 0.f};
            if (!first && e < E) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (rr + i < R) d[i] = ap[(size_t)i * E];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (4 * q < nb) d = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bv[q][ct], d, 0, 0, 0);
            if (e < E) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (rr + i < R) ap[(size_t)i * E] = d[i];
            }
        }
    }
}

extern "C" int tmg_tspec_block(const void* tm, const void* ring, void* acc, const int64_t* dims, hipStream_t st) {
    const int64_t E = dims[0], Tn = dims[1], NF = dims[2], n0 = dims[3], nb = dims[4], first = dims[5];
    if (E < 1 || Tn < 2 || NF < 1 || NF > Tn / 2 + 1 || n0 < 0 || nb < 1 || nb > TSPEC_RING || n0 + nb > Tn) return -1;
    const int64_t R = 2 * NF + 1, RP = (R + 15) / 16 * 16;
    if (E >= (1ll << 40) || R * E >= (1ll << 44) || Tn >= (1ll << 24)) return -2;
    if (!tm || !ring || !acc) return -3;
    const int64_t blocks = (E + 255) / 256;
    if (blocks >= (1ll << 31)) return -2;
    hipLaunchKernelGGL(tspec_block_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const float*)tm, (const float*)ring, (float*)acc,
                       (size_t)E, (int)R, (int)RP, (int)n0, (int)nb, (int)(first != 0));
    TMG_CHECK_LAUNCH();
    return 0;
}

__global__ __launch_bounds__(256) void tspec_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ cst,
                                                             float* __restrict__ psd_mean, float* __restrict__ psd_std, int S, int B,
                                                             int C, int HW, int NF, float inv_t) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int k = blockIdx.y, bc = blockIdx.z;
    if (p >= HW) return;
    const size_t hw = (size_t)HW;
    const size_t E = (size_t)S * B * C * hw, ms = (size_t)B * C * hw;
    const float gr = cst[k], gi = cst[NF + k], ck = cst[2 * NF + k];
    const float* are = acc + (size_t)k * E + (size_t)bc * hw + p;
    const float* aim = are + (size_t)NF * E;
    const float* asum = acc + (size_t)(2 * NF) * E + (size_t)bc * hw + p;
    float mean = 0.f, m2 = 0.f;
    for (int m = 0; m < S; ++m) {
        const size_t o = (size_t)m * ms;
        const float sm = asum[o];
        const float re = tmg_fourier_coef(are[o], sm, inv_t, gr), im = tmg_fourier_coef(aim[o], sm, inv_t, gi);
        const float P = ck * (re * re + im * im);
        const float d = P - mean;
        mean += d * (1.f / (float)(m + 1));
        m2 += d * (P - mean);
    }
    const int b = bc / C, c = bc - b * C;
    const size_t o = (((size_t)b * NF + k) * C + c) * hw + p;
    psd_mean[o] = mean;
    psd_std[o] = sqrtf(fmaxf(m2, 0.f) * (1.f / (float)S));
}

extern "C" int tmg_tspec_finalize(const void* acc, const void* cst, void* psd_mean, void* psd_std, const int64_t* dims, const float* fl,
                                  hipStream_t st) {
    const int64_t S = dims[0], B = dims[1], C = dims[2], HW = dims[3], NF = dims[4];
    if (S < 1 || B < 1 || C < 2 || C > TSPEC_MAXC || HW < 1 || NF < 1) return -1;
    if (!(fl[0] > 0.f) || !(fl[0] <= 0.5f)) return -1;
    if (HW >= (1ll << 31) - 256 || B * C > 65535 || NF > 65535 || S >= (1ll << 30)) return -2;
    if (S * B * C * HW >= (1ll << 40) || (2 * NF + 1) * S * B * C * HW >= (1ll << 44) || B * NF * C * HW >= (1ll << 40)) return -2;
    if (!acc || !cst || !psd_mean || !psd_std) return -3;
    dim3 grid((unsigned)((HW + 255) / 256), (unsigned)NF, (unsigned)(B * C));
    hipLaunchKernelGGL(tspec_finalize_kernel, grid, dim3(256), 0, st, (const float*)acc, (const float*)cst, (float*)psd_mean,
                       (float*)psd_std, (int)S, (int)B, (int)C, (int)HW, (int)NF, fl[0]);
    TMG_CHECK_LAUNCH();
    return 0;
}
