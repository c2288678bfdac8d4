// Spectral POD of sampled roll-outs (tmg_ops.EnsembleSpod / utils.modelPredSpod): the members stand where Welch's blocks stand.  The
// operand is tmg_tspec_block's accumulator acc [2 NF + 1][R][B][C][HW] over R = S + 1 rows (the S members, then the target): per row m,
// bin k, channel c and pixel p the Fourier coefficient of the windowed series, tmg_fourier_coef of tmg_dft.h (which is also
// tspec_finalize_kernel's):
//   xbar = acc[2 NF] * fl(1 / Tn),  Re X_m = acc[k] - xbar G_re,  Im X_m = acc[NF + k] - xbar G_im
//   spod_csd_kernel<DIAG>   the Gram blocks of tmg_symgram.h over the planes (case, bin), the walk over this file's rows: the real Gram
//                           matrix of the 2 R rows Z = [Re X_0 .. Re X_{R-1}; Im X_0 .. Im X_{R-1}] over the Cg HW elements of the
//                           selected channels, its partial blocks into the workspace, no atomics.  The upper triangle holds RR, II and
//                           the full RI block
//   symgram_reduce_kernel   (tmg_symgram.h) P > 1: the P slices' partials added in slice order (fp32)
//   spod_combine_kernel     csd_raw [B][NB][2][R][R]: raw0[m][n] = RR[lo][hi] + II[lo][hi] (lo, hi = min, max of m, n),
//                           raw1[m][n] = RI[m][n] - RI[n][m], one fp32 addition each: raw0 is bitwise symmetric, raw1 bitwise
//                           antisymmetric with an exactly zero diagonal
//   spod_modes_kernel       modes [B][NB][2 J][Cg][HW] = w [16 x 2 SP] Z [2 SP rows], the weights built on the host from the
//                           eigenvectors
//
// Layout and sum order of spod_csd_kernel: tmg_symgram.h, with Z = 2 R rows per plane and one pass per selected channel, in the order
// given, so that the plan (tmg_ens_spod_plan) reports L = Cg SL.  What is this file's own: a row's fragment is formed from the
// coefficient plane and the sum plane (two 64-byte runs, float4 loads when the rows are 16-byte aligned); the row pointers are formed
// before the loops, so that the inner loop holds loads, the correction and MFMAs only.  Roundings of one csd_raw entry beside L + P
// (tests/spod_cases.py counts them): 2 per operand for the correction (xbar G, then the subtraction; xbar itself is one more, counted
// with them as 3 per operand in the tests' bound) and 1 for the combine.
//
// spod_modes_kernel has tspec_block_kernel's shape: the weights are the A fragment (A[i = row r][k = q]), Z the B fragment, the D
// columns are consecutive pixels, so the stores run in 64-byte runs.  A wave owns 64 consecutive pixels of one channel (four column
// tiles); step qs contracts q = 4 qs .. 4 qs + 3, lane group lq holding q = 4 qs + lq: first the SP / 4 steps of the real parts, then
// those of the imaginary parts, the row pointers advanced by one constant per step.  Every output element is one fmaf chain in q order.
// No float atomics anywhere: the same inputs give the same bits.
#include "tmg_dft.h"
#include "tmg_symgram.h"
#include "tmglow_hip.h"
#include "tmglow_hip_spod.h"

#define SPOD_MAXC 4
#define SPOD_MAXS 255
#define SPOD_MAXB 16                     // bins of one call
#define SPOD_MAXJ 8

struct SpodSel {
    int bin[SPOD_MAXB];
    int ch[SPOD_MAXC];
};

// the shared plan for the 2 R rows and the B NB planes, and what this file adds: L, vec, MB
struct SpodPlan {
    SymgramPlan g;
    int64_t L, vec, MB;
};

static SpodPlan spod_plan(int64_t S, int64_t B, int64_t Cg, int64_t HW, int64_t NB, int64_t addr) {
    SpodPlan q;
    q.g = symgram_plan(2 * (S + 1), B * NB, HW);
    q.L = Cg * q.g.SL;
    q.vec = (HW % 4 == 0 && (addr & 15) == 0) ? 1 : 0;
    q.MB = (HW + 255) / 256;
    return q;
}

// The fragment of one row of Z for this lane's run of 16 pixels p0 .. p0 + 15: x - (s inv_t) g, 0 beyond HW and for a row that does not
// exist.  xrow: the coefficient plane's row (re_k or im_k), srow: the sum plane's, both at pixel 0 of the channel.
__device__ __forceinline__ void spod_frag(float (&f)[16], const float* __restrict__ xrow, const float* __restrict__ srow, bool live, int p0,
                                          int HW, bool vec, float g, float inv_t) {
#pragma clang fp contract(off)
#pragma unroll
    for (int s = 0; s < 16; ++s) f[s] = 0.f;
    if (!live || p0 >= HW) return;
    if (vec && p0 + 16 <= HW) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(xrow + p0 + 4 * q);
            const float4 t = *reinterpret_cast<const float4*>(srow + p0 + 4 * q);
            f[4 * q] = tmg_fourier_coef(v.x, t.x, inv_t, g);
            f[4 * q + 1] = tmg_fourier_coef(v.y, t.y, inv_t, g);
            f[4 * q + 2] = tmg_fourier_coef(v.z, t.z, inv_t, g);
            f[4 * q + 3] = tmg_fourier_coef(v.w, t.w, inv_t, g);
        }
    } else {
#pragma unroll
        for (int s = 0; s < 16; ++s)
            if (p0 + s < HW) f[s] = tmg_fourier_coef(xrow[p0 + s], srow[p0 + s], inv_t, g);
    }
}

// NTL: the 16-row tiles of a macro-tile that the instance holds, 4, or 1 for 2 R <= 16 (the partial is then [4 D registers][64 lanes])
template <bool DIAG, int NTL>
__global__ __launch_bounds__(256) void spod_csd_kernel(const float* __restrict__ acc, const float* __restrict__ cst, float* __restrict__ ws,
                                                       int R, int B, int C, int HW, int NF, int NB, int Cg, int SL, int P, int NT, int vec,
                                                       float inv_t, SpodSel sel) {
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, l16 = l & 15, kq = l >> 4;
    const int slice = blockIdx.x, bz = blockIdx.z;
    const int b = bz / NB, kb = bz - b * NB;
    int k = 0;
#pragma unroll
    for (int q = 0; q < SPOD_MAXB; ++q)
        if (q == kb) k = sel.bin[q];
    const int Z = 2 * R;
    const SymgramTile tl = symgram_tile<DIAG, NTL>(Z, NT);
    const int I = tl.I, J = tl.J, nti = tl.nti, ntj = tl.ntj;
    const size_t hw = (size_t)HW, E = (size_t)R * B * C * hw;
    const float gre = cst[k], gim = cst[NF + k];
    const float* sum0 = acc + (size_t)(2 * NF) * E;
    // this lane's rows: the coefficient plane's row, the sum plane's row (both at channel 0 of case b), the G part, whether it exists
    const float* xa[NTL];
    const float* sa[NTL];
    float ga[NTL];
    bool la[NTL];
    const float* xb[NTL];
    const float* sb[NTL];
    float gb[NTL];
    bool lb[NTL];
#pragma unroll
    for (int t = 0; t < NTL; ++t) {
        const int za = I * SYMGRAM_MT + 16 * t + l16, zb = J * SYMGRAM_MT + 16 * t + l16;
        la[t] = t < nti && za < Z;
        lb[t] = t < ntj && zb < Z;
        const int zac = la[t] ? za : 0, zbc = lb[t] ? zb : 0;
        const int ima = zac >= R, imb = zbc >= R;
        const size_t oa = ((size_t)(zac - ima * R) * B + b) * C * hw, ob = ((size_t)(zbc - imb * R) * B + b) * C * hw;
        xa[t] = acc + (size_t)(ima ? NF + k : k) * E + oa;
        sa[t] = sum0 + oa;
        ga[t] = ima ? gim : gre;
        xb[t] = acc + (size_t)(imb ? NF + k : k) * E + ob;
        sb[t] = sum0 + ob;
        gb[t] = imb ? gim : gre;
    }
    f32x4 d[NTL][NTL];
#pragma unroll
    for (int it = 0; it < NTL; ++it)
#pragma unroll
        for (int jt = 0; jt < NTL; ++jt) d[it][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int pbeg = slice * SL, pend = min(HW, pbeg + SL);
    for (int cg = 0; cg < Cg; ++cg) {
        int c = 0;
#pragma unroll
        for (int q = 0; q < SPOD_MAXC; ++q)
            if (q == cg) c = sel.ch[q];
        const size_t co = (size_t)c * hw;
        for (int pc = pbeg + wave * SYMGRAM_CHUNK; pc < pend; pc += 4 * SYMGRAM_CHUNK) {
            const int p0 = pc + kq * 16;
            float fa[NTL][16];
#pragma unroll
            for (int it = 0; it < NTL; ++it) spod_frag(fa[it], xa[it] + co, sa[it] + co, la[it], p0, HW, vec != 0, ga[it], inv_t);
#pragma unroll
            for (int jt = 0; jt < NTL; ++jt) {
                float fb[16];
                if (DIAG) {
#pragma unroll
                    for (int s = 0; s < 16; ++s) fb[s] = fa[jt][s];
                } else {
                    spod_frag(fb, xb[jt] + co, sb[jt] + co, lb[jt], p0, HW, vec != 0, gb[jt], inv_t);
                }
#pragma unroll
                for (int it = 0; it < NTL; ++it) {
                    if ((!DIAG || it <= jt) && it < nti && jt < ntj) {
#pragma unroll
                        for (int s = 0; s < 16; ++s) d[it][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[it][s], fb[s], d[it][jt], 0, 0, 0);
                    }
                }
            }
        }
    }
    symgram_store<DIAG, NTL>(d, tl, ws, P, NT);
}

// one thread per entry (m, n) of a (b, bin) plane: csd_raw [B NB][2][R][R]
__global__ __launch_bounds__(256) void spod_combine_kernel(const float* __restrict__ G, float* __restrict__ raw, int R, int NT, int part) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= R * R) return;
    const int m = e / R, n = e - m * R;
    const int NP = NT * (NT + 1) / 2;
    const float* Gp = G + (size_t)blockIdx.y * NP * part;
    const int lo = min(m, n), hi = max(m, n);
    const float rr = Gp[symgram_at(lo, hi, NT, part)], ii = Gp[symgram_at(R + lo, R + hi, NT, part)];
    const float rimn = Gp[symgram_at(m, R + n, NT, part)], rinm = Gp[symgram_at(n, R + m, NT, part)];
    float* o = raw + (size_t)blockIdx.y * 2 * R * R + e;
    o[0] = rr + ii;
    o[(size_t)R * R] = rimn - rinm;
}

__global__ __launch_bounds__(256) void spod_modes_kernel(const float* __restrict__ acc, const float* __restrict__ cst,
                                                         const float* __restrict__ w, float* __restrict__ out, int S, int R, int B, int C,
                                                         int HW, int NF, int NB, int Cg, int J, float inv_t, SpodSel sel) {
#pragma clang fp contract(off)
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, l16 = l & 15, lq = l >> 4;
    const int p0 = (blockIdx.x * 4 + wave) * 64;                           // the wave's first pixel
    if (p0 >= HW) return;                                                  // the whole wave is beyond the end
    const int cg = blockIdx.y, bz = blockIdx.z;
    const int b = bz / NB, kb = bz - b * NB;
    int k = 0, c = 0;
#pragma unroll
    for (int q = 0; q < SPOD_MAXB; ++q)
        if (q == kb) k = sel.bin[q];
#pragma unroll
    for (int q = 0; q < SPOD_MAXC; ++q)
        if (q == cg) c = sel.ch[q];
    const int SP = (S + 3) & ~3, QP = 2 * SP;
    const size_t hw = (size_t)HW, ms = (size_t)B * C * hw, E = (size_t)R * ms;
    const size_t o0 = ((size_t)b * C + c) * hw + p0 + l16;                 // member 0, this lane's pixel of column tile 0
    const float* wrow = w + ((size_t)bz * 16 + l16) * QP + lq;             // A[i = l16][k = lq] of step 0
    bool pv[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) pv[ct] = p0 + l16 + 16 * ct < HW;
    f32x4 d[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) d[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int part = 0; part < 2; ++part) {
        const float g = cst[part * NF + k];
        const float* xp = acc + (size_t)(part * NF + k) * E + o0 + (size_t)lq * ms;
        const float* sp = acc + (size_t)(2 * NF) * E + o0 + (size_t)lq * ms;
        for (int q = lq; q < SP; q += 4) {
            const float a = *wrow;
            float bv[4];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) bv[ct] = (q < S && pv[ct]) ? tmg_fourier_coef(xp[16 * ct], sp[16 * ct], inv_t, g) : 0.f;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) d[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[ct], d[ct], 0, 0, 0);
            wrow += 4;
            xp += 4 * ms;
            sp += 4 * ms;
        }
    }
    float* op = out + (((size_t)bz * 2 * J + 4 * lq) * Cg + cg) * hw + p0 + l16;   // D rows 4 lq + i, column l16
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * lq + i < 2 * J && pv[ct]) op[(size_t)i * Cg * hw + 16 * ct] = d[ct][i];
}

extern "C" int tmg_ens_spod_plan(const int64_t* dims, int64_t* plan) {
    const int64_t S = dims[0], B = dims[1], Cg = dims[2], HW = dims[3], NB = dims[4], addr = dims[5];
    if (S < 1 || S > SPOD_MAXS || B < 1 || HW < 1 || Cg < 1 || Cg > SPOD_MAXC || NB < 1 || NB > SPOD_MAXB) return -1;
    if (HW >= (1ll << 31) - 256 || B * NB > 65535 || (S + 1) * B * SPOD_MAXC * HW >= (1ll << 40)) return -2;
    if (!plan) return -3;
    const SpodPlan q = spod_plan(S, B, Cg, HW, NB, addr);
    plan[0] = q.g.P;
    plan[1] = q.L;
    plan[2] = q.g.NP;
    plan[3] = q.g.ws;
    plan[4] = q.g.SL;
    plan[5] = q.g.NT;
    plan[6] = q.g.part;
    plan[7] = q.vec;
    plan[8] = q.MB;
    return 0;
}

// the checks both launchers share; fills sel
static int spod_check(const int64_t* bins, const int64_t* channels, const int64_t* dims, SpodSel& sel) {
    const int64_t S = dims[0], B = dims[1], C = dims[2], HW = dims[3], NF = dims[4], Tn = dims[5], NB = dims[6], Cg = dims[7];
    if (S < 1 || S > SPOD_MAXS || B < 1 || HW < 1 || C < 2 || C > SPOD_MAXC || Cg < 1 || Cg > C || NB < 1 || NB > SPOD_MAXB) return -1;
    if (NF < 2 || Tn < 2 || NF > Tn / 2 + 1) return -1;
    if (HW >= (1ll << 31) - 256 || B * NB > 65535 || (S + 1) * B * C * HW >= (1ll << 40) || (2 * NF + 1) * (S + 1) * B * C * HW >= (1ll << 44) ||
        Tn >= (1ll << 24))
        return -2;
    if (!bins || !channels) return -3;
    for (int q = 0; q < SPOD_MAXB; ++q) sel.bin[q] = 1;
    for (int q = 0; q < SPOD_MAXC; ++q) sel.ch[q] = 0;
    for (int64_t q = 0; q < NB; ++q) {
        if (bins[q] < 1 || bins[q] >= NF || (q > 0 && bins[q] <= bins[q - 1])) return -1;
        sel.bin[q] = (int)bins[q];
    }
    bool used[SPOD_MAXC] = {false, false, false, false};
    for (int64_t q = 0; q < Cg; ++q) {
        if (channels[q] < 0 || channels[q] >= C || used[channels[q]]) return -1;
        used[channels[q]] = true;
        sel.ch[q] = (int)channels[q];
    }
    return 0;
}

extern "C" int tmg_ens_spod_csd(const void* acc, const void* cst, const int64_t* bins, const int64_t* channels, void* ws, void* csd_raw,
                                const int64_t* dims, hipStream_t st) {
    SpodSel sel;
    const int rc = spod_check(bins, channels, dims, sel);
    if (rc != 0) return rc;
    const int64_t S = dims[0], B = dims[1], C = dims[2], HW = dims[3], NF = dims[4], Tn = dims[5], NB = dims[6], Cg = dims[7],
                  ws_floats = dims[8];
    const int64_t R = S + 1;
    const SpodPlan q = spod_plan(S, B, Cg, HW, NB, (int64_t)((uintptr_t)acc & 15));
    const SymgramPlan& g = q.g;
    if (g.ws >= (1ll << 40)) return -2;
    if (ws_floats < g.ws) return -1;
    if (!acc || !cst || !ws || !csd_raw) return -3;
    const float inv_t = (float)(1.0 / (double)Tn);
    SYMGRAM_LAUNCH(spod_csd_kernel, g, B * NB, st, (const float*)acc, (const float*)cst, (float*)ws, (int)R, (int)B, (int)C, (int)HW, (int)NF,
                   (int)NB, (int)Cg, (int)g.SL, (int)g.P, (int)g.NT, (int)q.vec, inv_t, sel);
    const float* G = symgram_reduce(g, B * NB, (float*)ws, st);
    TMG_CHECK_LAUNCH();
    hipLaunchKernelGGL(spod_combine_kernel, dim3((unsigned)((R * R + 255) / 256), (unsigned)(B * NB)), dim3(256), 0, st, G, (float*)csd_raw,
                       (int)R, (int)g.NT, (int)g.part);
    TMG_CHECK_LAUNCH();
    return 0;
}

extern "C" int tmg_ens_spod_modes(const void* acc, const void* cst, const int64_t* bins, const int64_t* channels, const void* w, void* modes,
                                  const int64_t* dims, hipStream_t st) {
    SpodSel sel;
    const int rc = spod_check(bins, channels, dims, sel);
    if (rc != 0) return rc;
    const int64_t S = dims[0], B = dims[1], C = dims[2], HW = dims[3], NF = dims[4], Tn = dims[5], NB = dims[6], Cg = dims[7], J = dims[8];
    if (J < 1 || J > SPOD_MAXJ) return -1;
    if (B * NB * 2 * J * Cg * HW >= (1ll << 40)) return -2;
    if (!acc || !cst || !w || !modes) return -3;
    const float inv_t = (float)(1.0 / (double)Tn);
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)Cg, (unsigned)(B * NB));
    hipLaunchKernelGGL(spod_modes_kernel, grid, dim3(256), 0, st, (const float*)acc, (const float*)cst, (const float*)w, (float*)modes,
                       (int)S, (int)(S + 1), (int)B, (int)C, (int)HW, (int)NF, (int)NB, (int)Cg, (int)J, inv_t, sel);
    TMG_CHECK_LAUNCH();
    return 0;
}
