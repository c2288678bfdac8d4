// Energy score and member distances of sampled roll-outs (tmg_ops.EnsembleEnergy / utils.modelPredEnergy): the score of every member as
// ONE vector over the pixels, which the per-pixel scores of tmg_scores.hip cannot see.  Per case b, kept step and channel c the rows are
// the S raw normalised members x_0..x_{S-1} (the planar buffer xs [S][B][C][HW] that tmg_ens_score_store fills) and the normalised target
// x_S := y (read from its NHWC channel slice), R = S + 1 rows, centred about the members' mean r (the target is not in it):
//   e_m = x_m - r,   G_c[m][n] = sum_p e_m(c, p) e_n(c, p)                     the Gram matrix over the pixels, on the fp32 matrix pipe
//   d2_g[m][n] = max(0, sum_{c in g} a_c^2 (G_c[m][m] + G_c[n][n] - 2 G_c[m][n]))   per channel group g (channels of one unit)
// a_c = u[b][c] out_std[c] > 0; out_mu cancels.  Centring changes no distance: it makes G_mm + G_nn - 2 G_mn cancel against the spread
// of the members, not against the magnitude of the field.
//   ens_gram_mean_kernel       r [B][C][HW] = (x_0 + x_1 + .. + x_{S-1}, sequential fp32 in member order) * fl(1 / S)
//   ens_gram_kernel<DIAG>      the Gram blocks of tmg_symgram.h over the planes (case, channel): the walk over this file's rows between
//                              that header's pair decode and its hand-over and store; partial blocks into the workspace, no atomics
//   symgram_reduce_kernel      (tmg_symgram.h) P > 1: the P slices' partials added in slice order (fp32)
//   ens_gram_finalize_kernel   d2, dist = sqrt(d2), the means of the distances (fp64), the two argmins, traj_dist2 += d2 on timed steps;
//                              <true>: the same sums and argmins on sqrt(traj_dist2)
//
// Layout and sum order of ens_gram_kernel: tmg_symgram.h, with Z = R rows per plane and one pass over the pixels, so that the plan
// (tmg_ens_gram_plan) reports L = SL.  What is this file's own: a row's run of 16 pixels is four float4 loads when HW is a multiple of 4;
// the mean's run is loaded once per chunk and serves every row; r is subtracted when the fragment is built (one rounding per operand).
// Roundings of one d2 entry beside L + P, which the tests' rounding count is derived from (tests/energy_cases.py): 2 operand roundings
// (x - r), 2 combining additions (G_mm + G_nn, then - 2 G_mn; the doubling is exact), 2 for the scale (a_c^2 rounded once from fp64, one
// product), up to 3 additions over the channels of a group, 1 for the second-order terms: c = 10.  The sums over dist are fp64.
// No float atomics anywhere: the same inputs give the same bits, for every chunking of the members.
#include "tmg_symgram.h"
#include "tmglow_hip.h"

#define GRAM_MAXC 4
#define GRAM_MAXS 1024

struct GramGroups {
    int cnt[GRAM_MAXC];
    int ch[GRAM_MAXC][GRAM_MAXC];
};

__global__ __launch_bounds__(256) void ens_gram_mean_kernel(const float* __restrict__ xs, float* __restrict__ r, int S, size_t ms, int HW,
                                                            float inv_s) {
#pragma clang fp contract(off)
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const size_t o = (size_t)blockIdx.y * HW + p;
    float a = xs[o];
    for (int m = 1; m < S; ++m) a += xs[(size_t)m * ms + o];
    r[o] = a * inv_s;
}

// The fragment of one row for this lane's run of 16 pixels p0 .. p0 + 15: e = x - r, 0 beyond HW and for a row that does not exist.
// row < S: member `row` of xs (unit stride); row == S: the target (pixel stride tps).
__device__ __forceinline__ void gram_frag(float (&f)[16], const float* __restrict__ xrow, const float* __restrict__ trow, int tps, int row,
                                          int S, int p0, int HW, bool vec, const float (&rv)[16]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int s = 0; s < 16; ++s) f[s] = 0.f;
    if (row > S || p0 >= HW) return;
    if (row < S) {
        if (vec && p0 + 16 <= HW) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(xrow + p0 + 4 * q);
                f[4 * q] = v.x - rv[4 * q];
                f[4 * q + 1] = v.y - rv[4 * q + 1];
                f[4 * q + 2] = v.z - rv[4 * q + 2];
                f[4 * q + 3] = v.w - rv[4 * q + 3];
            }
        } else {
#pragma unroll
            for (int s = 0; s < 16; ++s)
                if (p0 + s < HW) f[s] = xrow[p0 + s] - rv[s];
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; ++s)
            if (p0 + s < HW) f[s] = trow[(size_t)(p0 + s) * tps] - rv[s];
    }
}

// NTL: the 16-row tiles of a macro-tile that the instance holds, 4, or 1 for R <= 16 (the partial is then [4 D registers][64 lanes])
template <bool DIAG, int NTL>
__global__ __launch_bounds__(256) void ens_gram_kernel(const float* __restrict__ xs, const float* __restrict__ tgt, int tps,
                                                       const float* __restrict__ r, float* __restrict__ ws, int S, int B, int C, int HW,
                                                       int SL, int P, int NT, int vec) {
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, l16 = l & 15, kq = l >> 4;
    const int slice = blockIdx.x, bc = blockIdx.z;
    const int b = bc / C, c = bc - b * C;
    const SymgramTile tl = symgram_tile<DIAG, NTL>(S + 1, NT);
    const int I = tl.I, J = tl.J, nti = tl.nti, ntj = tl.ntj;
    const size_t hw = (size_t)HW, ms = (size_t)B * C * hw;
    const float* xbc = xs + ((size_t)b * C + c) * hw;                      // member 0 of (b, c)
    const float* tbc = tgt + (size_t)b * hw * tps + c;
    const float* rbc = r + ((size_t)b * C + c) * hw;
    f32x4 acc[NTL][NTL];
#pragma unroll
    for (int it = 0; it < NTL; ++it)
#pragma unroll
        for (int jt = 0; jt < NTL; ++jt) acc[it][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int pbeg = slice * SL, pend = min(HW, pbeg + SL);
    for (int pc = pbeg + wave * SYMGRAM_CHUNK; pc < pend; pc += 4 * SYMGRAM_CHUNK) {
        const int p0 = pc + kq * 16;
        float rv[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) rv[s] = 0.f;
        if (vec && p0 + 16 <= HW) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(rbc + p0 + 4 * q);
                rv[4 * q] = v.x;
                rv[4 * q + 1] = v.y;
                rv[4 * q + 2] = v.z;
                rv[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int s = 0; s < 16; ++s)
                if (p0 + s < HW) rv[s] = rbc[p0 + s];
        }
        float fa[NTL][16];
#pragma unroll
        for (int it = 0; it < NTL; ++it) {
            const int row = I * SYMGRAM_MT + 16 * it + l16;
            gram_frag(fa[it], xbc + (size_t)min(row, S - 1) * ms, tbc, tps, it < nti ? row : S + 1, S, p0, HW, vec != 0, rv);
        }
#pragma unroll
        for (int jt = 0; jt < NTL; ++jt) {
            float fb[16];
            if (DIAG) {
#pragma unroll
                for (int s = 0; s < 16; ++s) fb[s] = fa[jt][s];
            } else {
                const int row = J * SYMGRAM_MT + 16 * jt + l16;
                gram_frag(fb, xbc + (size_t)min(row, S - 1) * ms, tbc, tps, jt < ntj ? row : S + 1, S, p0, HW, vec != 0, rv);
            }
#pragma unroll
            for (int it = 0; it < NTL; ++it) {
                if ((!DIAG || it <= jt) && it < nti && jt < ntj) {
#pragma unroll
                    for (int s = 0; s < 16; ++s) acc[it][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[it][s], fb[s], acc[it][jt], 0, 0, 0);
                }
            }
        }
    }
    symgram_store<DIAG, NTL>(acc, tl, ws, P, NT);
}

// One block per (group, case).  Thread m owns row m of the distance matrix (rows m, m + 256, ..): the sum of its distances to the
// members in column order (fp64) and its distance to the target; thread 0 then walks the members in order (fp64 sums, argmins with
// ties to the lowest index).  outf [5][B][Tk][Gn]: energy_score, energy_score_fair, target_dist_mean, pair_dist_mean, nearest_dist;
// outi [2][B][Tk][Gn]: medoid, nearest.
template <bool TRAJ>
__global__ __launch_bounds__(256) void ens_gram_finalize_kernel(const float* __restrict__ G, const float* __restrict__ a2,
                                                                float* __restrict__ traj, float* __restrict__ outf,
                                                                long long* __restrict__ outi, int S, int B, int C, int NT, int Tk, int t,
                                                                int t_before, int timed, int part, GramGroups gr) {
#pragma clang fp contract(off)
    __shared__ float dg[GRAM_MAXC][GRAM_MAXS + 1];
    __shared__ double rs[GRAM_MAXS], td[GRAM_MAXS];
    const int g = blockIdx.x, b = blockIdx.y, Gn = gridDim.x, R = S + 1;
    const int NP = NT * (NT + 1) / 2;
    int cnt = 0, ch[GRAM_MAXC] = {0, 0, 0, 0};
    float sc[GRAM_MAXC] = {0.f, 0.f, 0.f, 0.f};
    if (!TRAJ) {
#pragma unroll
        for (int q = 0; q < GRAM_MAXC; ++q)
            if (q == g) {
                cnt = gr.cnt[q];
#pragma unroll
                for (int k = 0; k < GRAM_MAXC; ++k) ch[k] = gr.ch[q][k];
            }
#pragma unroll
        for (int k = 0; k < GRAM_MAXC; ++k)
            if (k < cnt) {
                sc[k] = a2[b * C + ch[k]];
                const float* Gc = G + ((size_t)b * C + ch[k]) * NP * part;
                for (int m = threadIdx.x; m < R; m += 256) dg[k][m] = Gc[symgram_at(m, m, NT, part)];
            }
        __syncthreads();
    }
    float* tj = traj ? traj + ((size_t)b * Gn + g) * R * R : nullptr;
    for (int m = threadIdx.x; m < R; m += 256) {
        double rsum = 0.0, tdist = 0.0;
        for (int n = 0; n < R; ++n) {
            float d2 = 0.f;
            if (TRAJ) {
                d2 = tj[(size_t)m * R + n];
            } else {
                if (n != m) {
                    const int lo = min(m, n), hi = max(m, n);
                    const size_t at = symgram_at(lo, hi, NT, part);
                    float d = 0.f;
#pragma unroll
                    for (int k = 0; k < GRAM_MAXC; ++k)
                        if (k < cnt) {
                            const float gmn = G[((size_t)b * C + ch[k]) * NP * part + at];
                            const float s = dg[k][lo] + dg[k][hi];
                            const float q = s - 2.f * gmn;
                            const float v = sc[k] * q;
                            d = k == 0 ? v : d + v;
                        }
                    d2 = d < 0.f ? 0.f : d;                                // (not fmaxf: a NaN stays one)
                }
                if (timed) {
                    const size_t o = (size_t)m * R + n;
                    tj[o] = t_before > 0 ? tj[o] + d2 : d2;
                }
            }
            const float dist = sqrtf(d2);
            if (m < S) {
                if (n < S) rsum += (double)dist;
                else tdist = (double)dist;
            }
        }
        if (m < S) {
            rs[m] = rsum;
            td[m] = tdist;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double st = 0.0, sr = 0.0, best_r = rs[0], best_t = td[0];
        int med = 0, near = 0;
        for (int m = 0; m < S; ++m) {
            st += td[m];
            sr += rs[m];                                                   // every unordered pair twice
            if (rs[m] < best_r) {
                best_r = rs[m];
                med = m;
            }
            if (td[m] < best_t) {
                best_t = td[m];
                near = m;
            }
        }
        const double s = (double)S;
        const double tdm = st / s, pdm = sr / (s * s);
        const double pf = S > 1 ? sr / (s * (s - 1.0)) : 0.0;
        const size_t o = ((size_t)b * Tk + t) * Gn + g, n1 = (size_t)B * Tk * Gn;
        outf[o] = (float)(tdm - 0.5 * pdm);
        outf[n1 + o] = (float)(tdm - 0.5 * pf);
        outf[2 * n1 + o] = (float)tdm;
        outf[3 * n1 + o] = (float)pdm;
        outf[4 * n1 + o] = (float)best_t;
        outi[o] = med;
        outi[n1 + o] = near;
    }
}

extern "C" int tmg_ens_gram_plan(const int64_t* dims, int64_t* plan) {
    const int64_t S = dims[0], B = dims[1], C = dims[2], HW = dims[3];
    if (S < 1 || B < 1 || HW < 1 || C < 2 || C > GRAM_MAXC) return -1;
    if (S > GRAM_MAXS || HW >= (1ll << 31) - 256 || B * C > 65535 || S * B * C * HW >= (1ll << 40)) return -2;
    if (!plan) return -3;
    const SymgramPlan g = symgram_plan(S + 1, B * C, HW);
    plan[0] = g.P;
    plan[1] = g.SL;                                                        // L: one pass over the slice
    plan[2] = g.NP;
    plan[3] = g.ws;
    plan[4] = g.SL;
    plan[5] = g.NT;
    plan[6] = g.part;
    return 0;
}

// grp: GRAM_MAXC x GRAM_MAXC channel numbers, row g the channels of group g, -1 behind the last
static int gram_groups(const int64_t* grp, int64_t Gn, int64_t C, GramGroups& gr) {
    if (Gn < 1 || Gn > GRAM_MAXC) return -1;
    if (!grp) return 0;
    bool used[GRAM_MAXC] = {false, false, false, false};
    for (int g = 0; g < GRAM_MAXC; ++g) {
        gr.cnt[g] = 0;
        for (int k = 0; k < GRAM_MAXC; ++k) {
            const int64_t c = g < Gn ? grp[g * GRAM_MAXC + k] : -1;
            gr.ch[g][k] = 0;
            if (c == -1) continue;
            if (c < 0 || c >= C || used[c] || gr.cnt[g] != k) return -1;
            used[c] = true;
            gr.ch[g][k] = (int)c;
            gr.cnt[g] = k + 1;
        }
        if (g < Gn && gr.cnt[g] < 1) return -1;
    }
    return 0;
}

extern "C" int tmg_ens_gram_step(const void* xs, const void* target, const int64_t* t_d, const void* a2, const int64_t* grp, void* r,
                                 void* ws, int64_t ws_floats, void* traj, void* outf, void* outi, const int64_t* dims, hipStream_t st) {
    const int64_t S = dims[0], B = dims[1], HW = dims[2], C = dims[3], Gn = dims[4], Tk = dims[5], t = dims[6], t_before = dims[7],
                  flags = dims[8];
    const bool timed = flags & 1;
    if (S < 1 || B < 1 || HW < 1 || C < 2 || C > GRAM_MAXC || Tk < 1 || t < 0 || t >= Tk || t_before < 0) return -1;
    GramGroups gr;
    if (gram_groups(grp, Gn, C, gr) != 0) return -1;
    if (t_d && (t_d[0] < C || t_d[1] < 0 || t_d[1] + C > t_d[0])) return -1;
    if (S > GRAM_MAXS || HW >= (1ll << 31) - 256 || B * C > 65535 || S * B * C * HW >= (1ll << 40)) return -2;
    if (t_d && (t_d[0] >= (1ll << 31) || B * HW * t_d[0] >= (1ll << 40))) return -2;
    if (B * Tk * Gn >= (1ll << 40)) return -2;
    const SymgramPlan g = symgram_plan(S + 1, B * C, HW);
    if (g.ws >= (1ll << 40) || Gn * B * (S + 1) * (S + 1) >= (1ll << 40)) return -2;
    if (ws_floats < g.ws) return -1;
    if (!xs || !target || !t_d || !a2 || !grp || !r || !ws || !outf || !outi) return -3;
    if (timed && !traj) return -3;
    const int vec = (HW % 4 == 0 && (((uintptr_t)xs | (uintptr_t)r) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(ens_gram_mean_kernel, dim3((unsigned)((HW + 255) / 256), (unsigned)(B * C)), dim3(256), 0, st, (const float*)xs,
                       (float*)r, (int)S, (size_t)(B * C * HW), (int)HW, (float)(1.0 / (double)S));
    TMG_CHECK_LAUNCH();
    const float* tg = (const float*)target + t_d[1];
    SYMGRAM_LAUNCH(ens_gram_kernel, g, B * C, st, (const float*)xs, tg, (int)t_d[0], (const float*)r, (float*)ws, (int)S, (int)B, (int)C,
                   (int)HW, (int)g.SL, (int)g.P, (int)g.NT, vec);
    const float* G = symgram_reduce(g, B * C, (float*)ws, st);
    TMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(ens_gram_finalize_kernel<false>, dim3((unsigned)Gn, (unsigned)B), dim3(256), 0, st, G, (const float*)a2,
                       (float*)traj, (float*)outf, (long long*)outi, (int)S, (int)B, (int)C, (int)g.NT, (int)Tk, (int)t, (int)t_before,
                       timed ? 1 : 0, (int)g.part, gr);
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_gram_traj(const void* traj, void* outf, void* outi, const int64_t* dims, hipStream_t st) {
    const int64_t S = dims[0], B = dims[1], Gn = dims[2];
    if (S < 1 || B < 1 || Gn < 1 || Gn > GRAM_MAXC) return -1;
    if (S > GRAM_MAXS || B > 65535) return -2;
    if (!traj || !outf || !outi) return -3;
    GramGroups gr = {};
    hipLaunchKernelGGL(ens_gram_finalize_kernel<true>, dim3((unsigned)Gn, (unsigned)B), dim3(256), 0, st, (const float*)nullptr,
                       (const float*)nullptr, (float*)traj, (float*)outf, (long long*)outi, (int)S, (int)B, 0, 0, 1, 0, 0, 0, 0, gr);
    TMG_CHECK_LAUNCH();
    return 0;
}
