// One-dimensional line spectra of sampled roll-outs (tmg_ops.EnsembleLineSpectra / utils.modelPredLineSpectra): per line of the field
// the one-sided autospectra of the channels and the co- / quadrature spectrum of channels 0 and 1, of every step, of each member's
// time-mean coefficient and of its fluctuation about it (definitions: include/tmglow_hip_lspec.h).  The transform is linear, so the
// Fourier coefficient of a fluctuation is the fluctuation of the Fourier coefficient: a running complex mean and co-moment per
// member, line and mode give the fluctuation spectra in one pass over the roll-out.
//   lspec_chunk_kernel     a block owns 16 lines of one image: it un-normalises the C channels into LDS once (run-time pixel, line and
//                          point strides: rows and columns of the image are one kernel text; line stride N + 4 as spec_rows_kernel),
//                          its four waves share out the 16-mode tiles of the real operand [N][NQP] (cos, sin) and form Re X, Im X of
//                          all C channels on the fp32 matrix pipe (v_mfma_f32_16x16x4_f32), every operand fragment loaded once for the
//                          C channels.  Epilogue 1 (timed steps): the member's running mean and the F co-moment planes, every element
//                          owned by one lane; the tile's state is requested before the products, which hide its latency (measured:
//                          0.71 of the time of loading it in the epilogue, LAB_NOTES.md).  Epilogue 2: the tile's line sum of the
//                          planes of X, rows in register order, then the four lane groups in group order -> one partial per (image,
//                          line tile, plane, mode)
//   lspec_step_kernel      one thread per (case, plane, mode): the tiles' partials in tile order, then a sequential Welford over the
//                          members that continues from the stored state: the same bits for every chunking
//   lspec_finalize_kernel  once at the end: mean and population std over the members, in member order, of the fluctuation and of the
//                          mean-flow planes
// The MFMA lane maps and the side limit: tmg_dft.h.  No atomics and no data-dependent addressing anywhere.  Every kernel rounds each
// operation on its own (contraction off): a member that is constant in time leaves co-moments of exactly 0.
#include "tmg_dft.h"
#include "tmg_field.h"
#include "tmglow_hip_lspec.h"

#define LSPEC_MAXS 1024

// LDS: [C][16][N + 4] floats.  Lines past L are staged as zeros (never read from y) and never stored.
template <int C>
__global__ __launch_bounds__(256) void lspec_chunk_kernel(const float* __restrict__ y, int ps, const float* __restrict__ u,
                                                          const float* __restrict__ out_mu, const float* __restrict__ out_std,
                                                          const float* __restrict__ op, float* __restrict__ mean,
                                                          float* __restrict__ comom, float* __restrict__ part, int B, int L, int N,
                                                          int ls, int pstr, int m0, int t_before, int timed) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int F = C + 2;
    // line stride = 4 (mod 16): the 16 lines x 4 points of an A fragment fall into 64 different banks
    const int LS = N + 4;
    const int img = blockIdx.y, lt = blockIdx.x, LT = gridDim.x, l0 = lt * 16;
    const int b = img % B;
    const int NQ = N / 2 + 1, NQP = (NQ + 15) & ~15;
    float sc[C], mu[C], sd[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        sc[c] = u ? u[b * C + c] : 1.f;
        mu[c] = out_mu[c];
        sd[c] = out_std[c];
    }
    const float* yp = y + (size_t)img * L * N * ps;
    // consecutive threads walk along memory: along the line for rows (point stride 1), across the 16 lines for columns
    const bool rows = pstr == 1;
    for (int i = threadIdx.x; i < 16 * N; i += 256) {
        int r, n;
        if (rows) {
            r = i / N;
            n = i - r * N;
        } else {
            r = i & 15;
            n = i >> 4;
        }
        const int l = l0 + r;
        float v[C];
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = 0.f;
        if (l < L) {                                 // l < L and n < N: the pixel l ls + n pstr lies inside the image of L N pixels
            const float* q = yp + ((size_t)l * ls + (size_t)n * pstr) * ps;
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = tmg_unnorm_fma(q[c], sc[c], sd[c], mu[c]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) lds[(c * 16 + r) * LS + n] = v[c];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, l16 = l & 15, lq = l >> 4;
    const float* a0 = lds + l16 * LS + lq;
    const size_t plane = (size_t)N * NQP;
    const int member = m0 + img / B;
    // the wave that takes the odd tile out of four rotates with the block, so that the blocks a CU holds load its four SIMDs alike
    for (int qt = (wave + lt + img) & 3; qt < (NQP >> 4); qt += 4) {
        const float* fr = op + (size_t)lq * NQP + qt * 16 + l16;
        const float* fi = fr + plane;
        const int q = qt * 16 + l16;
        const bool qok = q < NQ;                    // the operand's padded columns are zero and never stored
        // the state this tile will update is requested before the products, which hide its latency (a first timed step reads none)
        float2 pm[4][C];
        float pc[4][F];
        const size_t fs = (size_t)L * NQ;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int line = l0 + lq * 4 + r;
            const bool live = timed && t_before > 0 && qok && line < L;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                pm[r][c] = make_float2(0.f, 0.f);
                if (live) pm[r][c] = ((const float2*)mean)[((((size_t)member * B + b) * C + c) * L + line) * NQ + q];
            }
#pragma unroll
            for (int f = 0; f < F; ++f) {
                pc[r][f] = 0.f;
                if (live) pc[r][f] = comom[(((size_t)member * B + b) * F * L + line) * NQ + q + f * fs];
            }
        }
        f32x4 re[C], im[C];
#pragma unroll
        for (int c = 0; c < C; ++c) re[c] = im[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < N; k0 += 16)         // N is a multiple of 16
#pragma unroll
        for (int k = k0; k < k0 + 16; k += 4) {
            const float b_r = fr[(size_t)k * NQP], b_i = fi[(size_t)k * NQP];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float a = a0[c * 16 * LS + k];
                re[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b_r, re[c], 0, 0, 0);
                im[c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b_i, im[c], 0, 0, 0);
            }
        }
        if (timed) {
            const float rn = 1.f / (float)(t_before + 1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int line = l0 + lq * 4 + r;
                if (!qok || line >= L) continue;
                float dor[C], doi[C], dnr[C], dni[C];    // X - Xbar before and after this step
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    float2* mp = (float2*)mean + ((((size_t)member * B + b) * C + c) * L + line) * NQ + q;
                    float2 m = pm[r][c];
                    dor[c] = re[c][r] - m.x;
                    doi[c] = im[c][r] - m.y;
                    m.x = m.x + dor[c] * rn;
                    m.y = m.y + doi[c] * rn;
                    dnr[c] = re[c][r] - m.x;
                    dni[c] = im[c][r] - m.y;
                    *mp = m;
                }
                float* cp = comom + (((size_t)member * B + b) * F * L + line) * NQ + q;
                float add[F];
#pragma unroll
                for (int c = 0; c < C; ++c) add[c] = dor[c] * dnr[c] + doi[c] * dni[c];
                add[C] = dor[0] * dnr[1] + doi[0] * dni[1];
                add[C + 1] = doi[0] * dnr[1] - dor[0] * dni[1];
#pragma unroll
                for (int f = 0; f < F; ++f) cp[f * fs] = pc[r][f] + add[f];
            }
        }
        float* pp = part + (((size_t)img * LT + lt) * F) * NQ + q;
#pragma unroll
        for (int f = 0; f < F; ++f) {
            const int cc = f < C ? f : 0;
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (f < C)
                    p[r] = re[cc][r] * re[cc][r] + im[cc][r] * im[cc][r];
                else if (f == C)
                    p[r] = re[0][r] * re[1][r] + im[0][r] * im[1][r];
                else
                    p[r] = im[0][r] * re[1][r] - re[0][r] * im[1][r];
            }
            const float s = ((p[0] + p[1]) + p[2]) + p[3];
            const float s0 = __shfl(s, l16), s1 = __shfl(s, l16 + 16), s2 = __shfl(s, l16 + 32), s3 = __shfl(s, l16 + 48);
            const float t = ((s0 + s1) + s2) + s3;
            if (lq == 0 && qok) pp[(size_t)f * NQ] = t;
        }
    }
}

static int lspec_shape(int64_t k, int64_t S, int64_t B, int64_t C, int64_t L, int64_t N) {
    if (k < 1 || S < 1 || B < 1 || L < 1 || C < 2 || C > 4 || k > S) return -1;
    if (!tmg_dft_side_ok(N)) return -1;
    const int64_t NQ = N / 2 + 1;
    if (S > LSPEC_MAXS || k * B > 65535 || (L + 15) / 16 > 65535) return -2;
    if (2 * S * B * C * L * NQ >= (1ll << 31) || S * B * (C + 2) * L * NQ >= (1ll << 31)) return -2;
    return 0;
}

extern "C" int tmg_ens_lspec_plan(const int64_t* dims, int64_t* out) {
    if (!dims || !out) return -3;
    const int64_t k = dims[0], S = dims[1], B = dims[2], C = dims[3], L = dims[4], N = dims[5];
    const int rc = lspec_shape(k, S, B, C, L, N);
    if (rc) return rc;
    const int64_t NQ = N / 2 + 1, NQP = (NQ + 15) / 16 * 16, LT = (L + 15) / 16, F = C + 2;
    out[0] = LT;                                     // the 16-line tiles of an image
    out[1] = NQP / 16;                               // the 16-mode tiles
    out[2] = LT;                                     // chunk grid x
    out[3] = k * B;                                  // chunk grid y: the images
    out[4] = 256;                                    // threads of every block
    out[5] = 64 * C * (N + 4);                       // LDS bytes: [C][16][N + 4] floats
    out[6] = NQ;
    out[7] = NQP;
    out[8] = k * B * LT * F * NQ;                    // floats of the partials [k B][LT][F][NQ]
    out[9] = 2 * S * B * C * L * NQ;                 // floats of the running means [S][B][C][L][NQ][2]
    out[10] = S * B * F * L * NQ;                    // floats of the co-moments [S][B][F][L][NQ]
    out[11] = 2 * N * NQP;                           // floats of the operand [2][N][NQP]
    return 0;
}

extern "C" int tmg_ens_lspec_chunk(const void* y, const int64_t* y_d, const void* u, const void* out_mu, const void* out_std,
                                   const void* op, void* mean, void* comom, void* part, const int64_t* dims, hipStream_t st) {
    if (!dims || !y_d) return -3;
    const int64_t k = dims[0], S = dims[1], B = dims[2], C = dims[3], L = dims[4], N = dims[5], ls = dims[6], pstr = dims[7],
                  m0 = dims[8], t_before = dims[9], flags = dims[10];
    int64_t plan[12];
    const int rc = tmg_ens_lspec_plan(dims, plan);
    if (rc) return rc;
    if (!((ls == N && pstr == 1) || (ls == 1 && pstr == L))) return -1;
    if (y_d[0] < C || y_d[1] < 0 || y_d[1] + C > y_d[0]) return -1;
    if (m0 < 0 || m0 + k > S || t_before < 0 || flags < 0 || flags > 1) return -1;
    if (k * B * L * N * y_d[0] >= (1ll << 40) || t_before >= (1ll << 24)) return -2;
    if (!y || !out_mu || !out_std || !op || !part) return -3;
    if ((flags & 1) && (!mean || !comom)) return -3;
    if (dims[11] < plan[8] || dims[14] < plan[11]) return -4;
    if ((flags & 1) && (dims[12] < plan[9] || dims[13] < plan[10])) return -4;
    const dim3 grid((unsigned)plan[2], (unsigned)plan[3]);
    const size_t smem = (size_t)plan[5];
#define LSPEC_LAUNCH(C_)                                                                                                          \
    do {                                                                                                                          \
        TMG_LDS_OPTIN(lspec_chunk_kernel<C_>);                                                                                    \
        hipLaunchKernelGGL(lspec_chunk_kernel<C_>, grid, dim3(256), smem, st, (const float*)y + y_d[1], (int)y_d[0],              \
                           (const float*)u, (const float*)out_mu, (const float*)out_std, (const float*)op, (float*)mean,          \
                           (float*)comom, (float*)part, (int)B, (int)L, (int)N, (int)ls, (int)pstr, (int)m0, (int)t_before,       \
                           (int)(flags & 1));                                                                                     \
    } while (0)
    if (C == 2)
        LSPEC_LAUNCH(2);
    else if (C == 3)
        LSPEC_LAUNCH(3);
    else
        LSPEC_LAUNCH(4);
#undef LSPEC_LAUNCH
    TMG_CHECK_LAUNCH();
    return 0;
}

__global__ __launch_bounds__(256) void lspec_step_kernel(const float* __restrict__ part, float* __restrict__ state,
                                                         float* __restrict__ mean_out, float* __restrict__ std_out, int k, int B,
                                                         int F, int L, int N, int n_before, int S, int Tk, int t, int last) {
#pragma clang fp contract(off)
    const int NQ = N / 2 + 1, LT = (L + 15) / 16;
    const int q = blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y / F, f = blockIdx.y - b * F;
    if (q >= NQ) return;
    const float aq = (q == 0 || q == N / 2) ? 1.f : 2.f;
    const float lines = (float)L;
    const size_t si = ((size_t)b * F + f) * NQ + q, half = (size_t)B * F * NQ;
    float mean = 0.f, m2 = 0.f;
    if (n_before > 0) {
        mean = state[si];
        m2 = state[half + si];
    }
    for (int j = 0; j < k; ++j) {
        const float* pp = part + (((size_t)(j * B + b) * LT) * F + f) * NQ + q;
        float E = 0.f;
        for (int i = 0; i < LT; ++i) E += pp[(size_t)i * F * NQ];     // the line tiles in tile order
        E = aq * E / lines;
        const float rn = 1.f / (float)(n_before + j + 1);
        const float d = E - mean;
        mean += d * rn;
        m2 += d * (E - mean);
    }
    if (last) {
        const size_t oi = (((size_t)b * Tk + t) * F + f) * NQ + q;
        mean_out[oi] = mean;
        std_out[oi] = sqrtf(fmaxf(m2, 0.f) * (1.f / (float)S));
    } else {
        state[si] = mean;
        state[half + si] = m2;
    }
}

extern "C" int tmg_ens_lspec_step(const void* part, void* state, void* mean_out, void* std_out, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], F = dims[2], L = dims[3], N = dims[4], n_before = dims[5], S = dims[6], Tk = dims[7],
                  t = dims[8], last = dims[9];
    if (k < 1 || B < 1 || L < 1 || S < 1 || Tk < 1 || F < 4 || F > 6 || n_before < 0) return -1;
    if (!tmg_dft_side_ok(N) || t < 0 || t >= Tk || last < 0 || last > 1) return -1;
    if (n_before + k > S || (last == 1) != (n_before + k == S)) return -1;
    if (B * F > 65535 || S > LSPEC_MAXS || k * B > 65535 || (L + 15) / 16 > 65535) return -2;
    if (B * Tk * F * (N / 2 + 1) >= (1ll << 31) || k * B * ((L + 15) / 16) * F * (N / 2 + 1) >= (1ll << 40)) return -2;
    if (!part) return -3;
    if (last ? (!mean_out || !std_out) : !state) return -3;
    if (n_before > 0 && !state) return -3;
    const int64_t NQ = N / 2 + 1;
    hipLaunchKernelGGL(lspec_step_kernel, dim3((unsigned)((NQ + 255) / 256), (unsigned)(B * F)), dim3(256), 0, st, (const float*)part,
                       (float*)state, (float*)mean_out, (float*)std_out, (int)k, (int)B, (int)F, (int)L, (int)N, (int)n_before, (int)S,
                       (int)Tk, (int)t, (int)last);
    TMG_CHECK_LAUNCH();
    return 0;
}

// One thread per element of [B][F][L][NQ].
__global__ __launch_bounds__(256) void lspec_finalize_kernel(const float* __restrict__ mean, const float* __restrict__ comom,
                                                             float* __restrict__ fluct_mean, float* __restrict__ fluct_std,
                                                             float* __restrict__ flow_mean, float* __restrict__ flow_std,
                                                             float* __restrict__ member_out, int S, int B, int C, int L, int N,
                                                             float steps) {
#pragma clang fp contract(off)
    const int NQ = N / 2 + 1, F = C + 2;
    const size_t n = (size_t)B * F * L * NQ;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const int q = (int)(e % NQ);
    const size_t lq = e / NQ;                        // (b F + f) L + line
    const int line = (int)(lq % L);
    const int bf = (int)(lq / L);
    const int b = bf / F, f = bf - b * F;
    const float aq = (q == 0 || q == N / 2) ? 1.f : 2.f;
    const int c0 = f < C ? f : 0, c1 = f < C ? f : 1;
    float am = 0.f, aq2 = 0.f, bm = 0.f, bq2 = 0.f;
    for (int m = 0; m < S; ++m) {
        const float rn = 1.f / (float)(m + 1);
        const float v = aq * comom[((((size_t)m * B + b) * F + f) * L + line) * NQ + q] / steps;
        if (member_out) member_out[((((size_t)b * S + m) * F + f) * L + line) * NQ + q] = v;
        float d = v - am;
        am += d * rn;
        aq2 += d * (v - am);
        const float2 x0 = ((const float2*)mean)[((((size_t)m * B + b) * C + c0) * L + line) * NQ + q];
        const float2 x1 = ((const float2*)mean)[((((size_t)m * B + b) * C + c1) * L + line) * NQ + q];
        const float w = aq * (f == C + 1 ? x0.y * x1.x - x0.x * x1.y : x0.x * x1.x + x0.y * x1.y);
        d = w - bm;
        bm += d * rn;
        bq2 += d * (w - bm);
    }
    const float rs = 1.f / (float)S;
    fluct_mean[e] = am;
    fluct_std[e] = sqrtf(fmaxf(aq2, 0.f) * rs);
    flow_mean[e] = bm;
    flow_std[e] = sqrtf(fmaxf(bq2, 0.f) * rs);
}

extern "C" int tmg_ens_lspec_finalize(const void* mean, const void* comom, void* fluct_mean, void* fluct_std, void* flow_mean,
                                      void* flow_std, void* member_out, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t S = dims[0], B = dims[1], C = dims[2], L = dims[3], N = dims[4], T = dims[5];
    if (T < 1) return -1;
    const int rc = lspec_shape(1, S, B, C, L, N);
    if (rc) return rc;
    if (T >= (1ll << 24)) return -2;
    if (!mean || !comom || !fluct_mean || !fluct_std || !flow_mean || !flow_std) return -3;
    const int64_t n = B * (C + 2) * L * (N / 2 + 1);
    hipLaunchKernelGGL(lspec_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)mean,
                       (const float*)comom, (float*)fluct_mean, (float*)fluct_std, (float*)flow_mean, (float*)flow_std,
                       (float*)member_out, (int)S, (int)B, (int)C, (int)L, (int)N, (float)T);
    TMG_CHECK_LAUNCH();
    return 0;
}
