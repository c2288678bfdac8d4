// Phase averages of sampled roll-outs on the shedding phase (tmg_ops.EnsemblePhase / utils.modelPredPhase): the triple decomposition
// u = U + u~ + u' of Reynolds & Hussain.  The phase of a row (a member of the chunk, or the step's target) is the angle of its two
// coefficients on a pair of the target's POD modes, which tmg_ens_pod_project has just left on the device; the circle is cut into NB
// equal sectors and every row's fluctuation about the target's time mean is added to the accumulators of its sector.
//   ens_phase_label_kernel        one thread per row: x = fl(g_i raw_i), y = fl(g_j raw_j); label -1 when fl(fl(x x) + fl(y y)) < thr,
//                                 else the sector of the angle of (x, y).  No transcendental: the quadrant from the signs, inside it
//                                 the count of the table tangents t_q with fl(t_q p) <= q, (p, q) = (|x|, |y|) in the quadrants that
//                                 open at the x axis and (|y|, |x|) in those that open at the y axis.  Every operation is rounded on
//                                 its own (no contraction), so a float32 host mirror gives the same label bit for bit
//   ens_phase_accum_kernel<C, V>  one block per (pixel tile, sector, case).  The block scans the k labels of its case (uniform over
//                                 the block: scalar loads and branches); with no row in its sector it returns without a write.
//                                 Otherwise every thread loads its Q = 2 C + 1 accumulator values FIRST, adds the matching rows in
//                                 member order and stores once:
//                                   d_c = fl(a_c fl(x_c - m_c));  planes: d_c (C), fl(d_c d_c) (C), fl(d_0 d_1)
// Because the running value is loaded before the first add, the fp32 additions into one accumulator element run "steps in order,
// members in order" whatever the chunking: bitwise reproducible, no atomics, no LDS, no partial sums.  Traffic: each row is read once
// (by the one sector block per tile that owns it; the other sector blocks read labels only), and per pixel tile and chunk at most
// min(NB, k) accumulator tiles are read and written.
//   V = 1: four consecutive pixels per thread, 16-byte loads of the rows (C float4 hold 4 pixels x C channels), of m and of the
//          accumulators: pixel stride == C, channel offset 0, HW a multiple of 4 and every base 16-byte aligned
//   V = 0: one pixel per thread, dword loads (channel slices of wider rows, ragged fields)
#include "tmg_common.h"
#include "tmglow_hip.h"

#define PHASE_MAXS 1024
#define PHASE_THREADS 256
#define PHASE_MAXTAN 7                   // NB / 4 - 1 tangents inside a quadrant, NB <= 32

struct PhaseTan {
    float t[PHASE_MAXTAN];
};

struct PhasePlan {
    int64_t tile, tiles, vec;
};

// vec_ok: the rows are dense (pixel stride C, channel offset 0) and every base is 16-byte aligned
static PhasePlan phase_plan(int64_t HW, int vec_ok) {
    PhasePlan g;
    g.vec = (vec_ok && HW % 4 == 0) ? 1 : 0;
    g.tile = g.vec ? 4 * PHASE_THREADS : PHASE_THREADS;
    g.tiles = (HW + g.tile - 1) / g.tile;
    return g;
}

__global__ __launch_bounds__(PHASE_THREADS) void ens_phase_label_kernel(const float* __restrict__ coef, long long cs, long long ms, int pi,
                                                                        int pj, const float* __restrict__ g, PhaseTan tt, float thr,
                                                                        int* __restrict__ lab, long long ls_c, long long ls_m, int k,
                                                                        int B, int NB) {
#pragma clang fp contract(off)
    const long long row = (long long)blockIdx.x * PHASE_THREADS + threadIdx.x;
    if (row >= (long long)k * B) return;
    const int s = (int)(row / B), b = (int)(row - (long long)s * B);
    const float* cp = coef + (size_t)b * cs + (size_t)s * ms;
    const float x = g[2 * b] * cp[pi], y = g[2 * b + 1] * cp[pj];
    const float xx = x * x, yy = y * y;
    const float r2 = xx + yy;
    int out = 0;                                                               // (0, 0) that passes the gate: sector 0
    if (r2 < thr) {
        out = -1;
    } else {
        const float ax = __builtin_fabsf(x), ay = __builtin_fabsf(y);
        const int nq = NB >> 2;
        int base = -1;
        float p = ax, q = ay;
        if (x > 0.f && y >= 0.f) {
            base = 0;
        } else if (x <= 0.f && y > 0.f) {
            base = nq, p = ay, q = ax;
        } else if (x < 0.f && y <= 0.f) {
            base = 2 * nq;
        } else if (x >= 0.f && y < 0.f) {
            base = 3 * nq, p = ay, q = ax;
        }
        if (base >= 0) {
            int cnt = 0;
#pragma unroll
            for (int i = 0; i < PHASE_MAXTAN; ++i) {
                const float e = tt.t[i] * p;
                cnt += (i < nq - 1 && e <= q) ? 1 : 0;
            }
            out = base + cnt;
        }
    }
    lab[(size_t)b * ls_c + (size_t)s * ls_m] = out;
}

template <int C, int V>
__global__ __launch_bounds__(PHASE_THREADS) void ens_phase_accum_kernel(const float* __restrict__ y, int ps, const int* __restrict__ lab,
                                                                        long long ls_c, long long ls_m, const float* __restrict__ a,
                                                                        const float* __restrict__ m, float* __restrict__ acc, int k, int B,
                                                                        int HW, int NB) {
#pragma clang fp contract(off)
    constexpr int Q = 2 * C + 1, PX = V ? 4 : 1;
    const int sector = blockIdx.y, b = blockIdx.z;
    const int* lb = lab + (size_t)b * ls_c;
    int any = 0;
    for (int s = 0; s < k; ++s) any |= lb[(size_t)s * ls_m] == sector ? 1 : 0;
    if (!any) return;                                                          // uniform: nothing of this chunk belongs here
    const long long p = ((long long)blockIdx.x * PHASE_THREADS + threadIdx.x) * PX;
    if (p >= HW) return;                                                       // (V: HW is a multiple of 4, so p + 3 < HW)
    const size_t hw = (size_t)HW;
    float av[C], mv[C][PX], r[Q][PX];
    const float* mp = m + (size_t)b * C * hw + p;
    float* ap = acc + ((size_t)b * NB + sector) * Q * hw + p;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        av[c] = a[b * C + c];
        if constexpr (V) {
            const float4 t = *reinterpret_cast<const float4*>(mp + c * hw);
            mv[c][0] = t.x, mv[c][1] = t.y, mv[c][2] = t.z, mv[c][3] = t.w;
        } else {
            mv[c][0] = mp[c * hw];
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if constexpr (V) {
            const float4 t = *reinterpret_cast<const float4*>(ap + q * hw);
            r[q][0] = t.x, r[q][1] = t.y, r[q][2] = t.z, r[q][3] = t.w;
        } else {
            r[q][0] = ap[q * hw];
        }
    }
    const size_t rs = (size_t)B * hw * ps;                                     // floats between two members of one case
    const float* yp = y + ((size_t)b * hw + (size_t)p) * ps;
    for (int s = 0; s < k; ++s) {
        if (lb[(size_t)s * ls_m] != sector) continue;                          // uniform
        const float* yr = yp + (size_t)s * rs;
        float f[PX * C];
        if constexpr (V) {                                                     // ps == C: 4 pixels x C channels are C float4
#pragma unroll
            for (int v = 0; v < C; ++v) {
                const float4 t = *reinterpret_cast<const float4*>(yr + 4 * v);
                f[4 * v] = t.x, f[4 * v + 1] = t.y, f[4 * v + 2] = t.z, f[4 * v + 3] = t.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) f[c] = yr[c];
        }
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            float d[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float t = f[j * C + c] - mv[c][j];
                d[c] = av[c] * t;
                const float dd = d[c] * d[c];
                r[c][j] = r[c][j] + d[c];
                r[C + c][j] = r[C + c][j] + dd;
            }
            const float uv = d[0] * d[1];
            r[2 * C][j] = r[2 * C][j] + uv;
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if constexpr (V) *reinterpret_cast<float4*>(ap + q * hw) = make_float4(r[q][0], r[q][1], r[q][2], r[q][3]);
        else ap[q * hw] = r[q][0];
    }
}

static int phase_sizes(int64_t S, int64_t B, int64_t C, int64_t HW, int64_t NB) {
    if (S < 1 || B < 1 || HW < 1 || C < 2 || C > 4 || NB < 4 || (NB <= 32 && NB != 4 && NB != 8 && NB != 16 && NB != 32)) return -1;
    if (NB > 32 || S > PHASE_MAXS || B > 65535 || HW >= (1ll << 31) - 4 * PHASE_THREADS || S * B * HW * C >= (1ll << 40) ||
        B * NB * (2 * C + 1) * HW >= (1ll << 40))
        return -2;
    return 0;
}

extern "C" int tmg_ens_phase_plan(const int64_t* dims, int64_t* plan) {
    if (!dims) return -3;
    const int64_t S = dims[0], B = dims[1], C = dims[2], HW = dims[3], NB = dims[4];
    const int rc = phase_sizes(S, B, C, HW, NB);
    if (rc != 0) return rc;
    if (!plan) return -3;
    const PhasePlan g = phase_plan(HW, 1);
    plan[0] = g.tile;
    plan[1] = g.tiles;
    plan[2] = NB;
    plan[3] = B;
    plan[4] = 0;
    plan[5] = g.vec;
    return 0;
}

extern "C" int tmg_ens_phase_label(const void* coef, const int64_t* c_d, const int64_t* pair, const void* g, const float* tab, void* lab,
                                   const int64_t* l_d, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], NB = dims[2];
    int rc = phase_sizes(k, B, 2, 1, NB);
    if (rc == -1) return rc;
    if (c_d && (c_d[0] < 0 || c_d[1] < 0)) return -1;
    if (l_d && (l_d[0] < 0 || l_d[1] < 0)) return -1;
    if (pair && (pair[0] < 0 || pair[1] < 0 || pair[0] == pair[1])) return -1;
    PhaseTan tt = {{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}};
    if (tab) {
        if (!(tab[0] >= 0.f) || !(tab[0] <= 3.0e38f)) return -1;               // the gate: finite, not negative
        float prev = 0.f;
        for (int i = 0; i < NB / 4 - 1 && NB <= 32; ++i) {                     // the tangents: finite, positive, increasing
            if (!(tab[1 + i] > prev) || !(tab[1 + i] <= 3.0e38f)) return -1;
            prev = tt.t[i] = tab[1 + i];
        }
    }
    if (rc != 0) return rc;
    if (pair && (pair[0] >= (1ll << 31) || pair[1] >= (1ll << 31))) return -2;
    if (c_d && (B * c_d[0] >= (1ll << 40) || k * c_d[1] >= (1ll << 40))) return -2;
    if (l_d && (B * l_d[0] >= (1ll << 40) || k * l_d[1] >= (1ll << 40))) return -2;
    if (!coef || !c_d || !pair || !g || !tab || !lab || !l_d) return -3;
    const int64_t rows = k * B;
    hipLaunchKernelGGL(ens_phase_label_kernel, dim3((unsigned)((rows + PHASE_THREADS - 1) / PHASE_THREADS)), dim3(PHASE_THREADS), 0, st,
                       (const float*)coef, (long long)c_d[0], (long long)c_d[1], (int)pair[0], (int)pair[1], (const float*)g, tt, tab[0],
                       (int*)lab, (long long)l_d[0], (long long)l_d[1], (int)k, (int)B, (int)NB);
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_phase_accum(const void* rows, const int64_t* t_d, const void* lab, const int64_t* l_d, const void* a, const void* m,
                                   void* acc, const int64_t* dims, hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], HW = dims[2], C = dims[3], NB = dims[4];
    int rc = phase_sizes(k, B, C, HW, NB);
    if (rc == -1) return rc;
    if (t_d && (t_d[1] < 0 || t_d[0] < t_d[1] + C)) return -1;
    if (l_d && (l_d[0] < 0 || l_d[1] < 0)) return -1;
    if (rc != 0) return rc;
    if (t_d && (t_d[0] >= (1ll << 31) || k * B * HW * t_d[0] >= (1ll << 40))) return -2;
    if (l_d && (B * l_d[0] >= (1ll << 40) || k * l_d[1] >= (1ll << 40))) return -2;
    if (!rows || !t_d || !lab || !l_d || !a || !m || !acc) return -3;
    const float* yr = (const float*)rows + t_d[1];
    const int dense = t_d[0] == C && t_d[1] == 0 && (((uintptr_t)yr | (uintptr_t)m | (uintptr_t)acc) & 15) == 0;
    const PhasePlan g = phase_plan(HW, dense);
    const dim3 grid((unsigned)g.tiles, (unsigned)NB, (unsigned)B);
#define PHASE_LAUNCH(C_, V_)                                                                                                          \
    hipLaunchKernelGGL((ens_phase_accum_kernel<C_, V_>), grid, dim3(PHASE_THREADS), 0, st, yr, (int)t_d[0], (const int*)lab,          \
                       (long long)l_d[0], (long long)l_d[1], (const float*)a, (const float*)m, (float*)acc, (int)k, (int)B, (int)HW, \
                       (int)NB)
    if (g.vec) {
        if (C == 2) PHASE_LAUNCH(2, 1);
        else if (C == 3) PHASE_LAUNCH(3, 1);
        else PHASE_LAUNCH(4, 1);
    } else {
        if (C == 2) PHASE_LAUNCH(2, 0);
        else if (C == 3) PHASE_LAUNCH(3, 0);
        else PHASE_LAUNCH(4, 0);
    }
#undef PHASE_LAUNCH
    TMG_CHECK_LAUNCH();
    return 0;
}
