// Probability densities of the flow quantities pooled over regions of the flow (tmg_ops.EnsemblePdfs / utils.modelPredPdfs): marginal
// histograms of up to 8 fields (a raw normalised channel, optionally centred; or the physical speed, vorticity, divergence) and joint
// histograms of up to 2 pairs of them, over up to 4 pixel boxes, for the members and (as a one-member chunk) for the target.  The
// definitions - values, edges, the bin index idx(d) = #{j : d >= e_j}, regions - are in include/tmglow_hip_pdf.h.
//   ens_pdf_count_kernel<DER>   one chunk of k whole members: one block takes a slice of SL pixels of one row (member, case), bins
//                               them into LDS histograms (int32, LDS integer atomics) and at the end issues one global integer
//                               atomicAdd per non-empty bin into the step's planes and, on a timed step, into the member's time plane
//                               and the pooled joint time plane.  DER = 1 also forms the derived fields.
// Integer sums do not depend on the order: every output is bitwise reproducible and independent of the chunking.  No float atomic,
// no scratch (every per-field array is indexed by compile-time constants in unrolled loops).
//
// Contention.  The divergence of a good surrogate, any field outside its range, and every smooth field (neighbouring pixels, which
// are neighbouring lanes, fall into the same bin) put many lanes of a wave on one LDS address, and the LDS serialises the lanes of
// one instruction that hit one address.  A private histogram per wave does not change that (the conflict is inside the wave), so the
// kernel aggregates instead: the lanes whose index equals the first active lane's are counted by a ballot and added once, the others
// add 1 each.  One round removes the whole wave in the one-bin extreme and costs a compare and a ballot in the spread extreme.
// Measured against four private per-wave histograms with plain adds (LAB_NOTES.md): up to 25 % faster on a one-bin input, within
// 3 % on a uniformly spread one, and a quarter of the LDS.
//
// The bin index.  The edge tables sit in LDS, with nb / (e_nb - e_0) of each.  An arithmetic guess (d - e_0) nb / (e_nb - e_0) is corrected by comparisons with the
// table until e_{g-1} <= d < e_g holds, so the result is the definition's count for any guess; on uniform edges the guess is off by
// at most one, and the correction is two reads.
// The 3x3 neighbours are read from global memory: tmg_ensemble.hip explains why an LDS tile does not pay for NHWC input with a
// run-time stride.
#include "tmg_field.h"
#include "tmglow_hip.h"

#define PDF_MAXC 4
#define PDF_MAXF 8
#define PDF_MAXP 2
#define PDF_MAXR 4
#define PDF_MAXNB 128
#define PDF_MAXNBJ 32
#define PDF_THREADS 256
#define PDF_PPT 4            // pixels per thread: a slice is 1024 pixels
#define PDF_LDS_MAX 65536

struct PdfArgs {
    int kind[PDF_MAXF];      // 0..3: channel; 4: speed; 5: vort; 6: div
    int pair[PDF_MAXP][2];
    int box[PDF_MAXR][4];    // x0, x1, y0, y1
};

struct PdfPlan {
    long long sl, nsl, lds, copies, instance, threads, blocks, ppt, marg, joint, ne, nje;
};

// dims = {k, B, H, W, F, nb, P, nbj, R, derived}; -> 0 and the plan, or the code
static int pdf_plan(const int64_t* dims, PdfPlan* q) {
    const int64_t k = dims[0], B = dims[1], H = dims[2], W = dims[3], F = dims[4], nb = dims[5], P = dims[6], nbj = dims[7], R = dims[8],
                  der = dims[9];
    if (k < 1 || B < 1 || H < 1 || W < 1 || F < 1 || F > PDF_MAXF || nb < 1 || nb > PDF_MAXNB || P < 0 || P > PDF_MAXP || R < 1 ||
        R > PDF_MAXR || der < 0 || der > 1)
        return -1;
    if (P > 0 && (nbj < 1 || nbj > PDF_MAXNBJ)) return -1;
    if (H >= (1ll << 31) || W >= (1ll << 31) || H * W >= (1ll << 31) - 1024 || k * B > 65535) return -2;
    const int64_t HW = H * W;
    q->ppt = PDF_PPT;
    q->sl = PDF_THREADS * q->ppt;
    q->nsl = (HW + q->sl - 1) / q->sl;
    q->ne = F * (nb + 1);
    q->nje = P * 2 * (nbj + 1) + F + 2 * P;                                    // the joint edges, then one guess scale per table
    q->marg = R * F * (nb + 2);
    q->joint = P ? R * P * (nbj + 2) * (nbj + 2) : 0;
    q->copies = 1;                                                             // one histogram per block: pdf_add aggregates instead
    q->lds = 4 * (q->ne + q->nje + q->copies * q->marg + q->joint);
    if (q->lds > PDF_LDS_MAX) return -2;                                       // (58 336 bytes at the largest sizes: never taken)
    q->instance = der;
    q->threads = PDF_THREADS;
    q->blocks = q->nsl * k * B;
    return 0;
}

extern "C" int tmg_ens_pdf_plan(const int64_t* dims, int64_t* plan) {
    if (!dims) return -3;
    PdfPlan q;
    const int rc = pdf_plan(dims, &q);
    if (rc) return rc;
    if (!plan) return -3;
    const long long v[8] = {q.sl, q.nsl, q.lds, q.copies, q.instance, q.threads, q.blocks, q.ppt};
    for (int i = 0; i < 8; ++i) plan[i] = v[i];
    return 0;
}

// Everything below rounds every operation on its own: the numpy float32 mirror of the tests reproduces the derived fields bit for bit.
#pragma clang fp contract(off)

// idx(d) = #{j in 0..n : d >= e[j]} for strictly increasing e[0..n] (LDS): a guess, corrected until e[g - 1] <= d < e[g]
__device__ __forceinline__ int pdf_index(const float* e, int n, float scale, float d) {
    float t = (d - e[0]) * scale;
    t = fminf(fmaxf(t, -1.f), (float)n);                                       // (a NaN becomes -1: the index stays inside the table)
    int g = (int)floorf(t) + 1;
    while (g <= n && d >= e[g]) ++g;
    while (g > 0 && d < e[g - 1]) --g;
    return g;
}

// one count into an LDS histogram: the lanes that share the first active lane's bin add once, the others one by one
__device__ __forceinline__ void pdf_add(int* h, int i) {
    const int lead = __builtin_amdgcn_readfirstlane(i);
    const bool same = i == lead;
    const unsigned long long m = __ballot(same);
    if (same) {
        if ((int)(__ffsll((long long)m) - 1) == (int)(threadIdx.x & 63)) atomicAdd(h + lead, (int)__popcll(m));
    } else {
        atomicAdd(h + i, 1);
    }
}

template <int DER>
__global__ __launch_bounds__(PDF_THREADS) void ens_pdf_count_kernel(
    const float* __restrict__ y, int ps, const float* __restrict__ u, const float* __restrict__ out_mu, const float* __restrict__ out_std,
    const float* __restrict__ cen, const float* __restrict__ edges, const float* __restrict__ jedges, int* __restrict__ step_count,
    int* __restrict__ step_joint, int* __restrict__ mtime, int* __restrict__ tjoint, long long ocs, long long jcs, int B, int Hh, int Ww,
    int C, int S, int m0, int F, int nb, int P, int nbj, int R, int flags, float rdx, float rdy, PdfArgs a) {
    extern __shared__ int lds[];
    const int tid = threadIdx.x;
    const int row = blockIdx.y;                                                // member j of the chunk, case b
    const int j = row / B, b = row - j * B;
    const int HW = Hh * Ww;
    const int ne = F * (nb + 1), nje0 = P * 2 * (nbj + 1), nje = nje0 + F + 2 * P, nm = R * F * (nb + 2), jb = (nbj + 2) * (nbj + 2), nj = P ? R * P * jb : 0;
    float* le = (float*)lds;                                                   // [F][nb + 1]
    float* lj = le + ne;                                                       // [P][2][nbj + 1]
    float* ls = lj + nje0;                                                     // [F] + [P][2]: n / (e_n - e_0) of every table
    int* hm = lds + ne + nje;                                                  // [R][F][nb + 2]
    int* hj = hm + nm;                                                         // [R][P][(nbj + 2)^2]
    for (int i = tid; i < ne; i += PDF_THREADS) le[i] = edges[(size_t)b * ne + i];
    for (int i = tid; i < nje0; i += PDF_THREADS) lj[i] = jedges[(size_t)b * nje0 + i];
    if (tid < F) {
        const float* e = edges + (size_t)b * ne + tid * (nb + 1);
        ls[tid] = (float)nb / (e[nb] - e[0]);
    } else if (tid < F + 2 * P) {
        const float* e = jedges + (size_t)b * nje0 + (tid - F) * (nbj + 1);
        ls[tid] = (float)nbj / (e[nbj] - e[0]);
    }
    for (int i = tid; i < nm + nj; i += PDF_THREADS) hm[i] = 0;
    __syncthreads();

    float sc0 = 1.f, sc1 = 1.f, mu0 = 0.f, mu1 = 0.f, sd0 = 1.f, sd1 = 1.f;
    bool sten = false;
    if (DER) {
        if (u) {
            sc0 = u[b * C];
            sc1 = u[b * C + 1];
        }
        mu0 = out_mu[0];
        mu1 = out_mu[1];
        sd0 = out_std[0];
        sd1 = out_std[1];
#pragma unroll
        for (int f = 0; f < PDF_MAXF; ++f) sten = sten || (f < F && a.kind[f] >= 5);
    }
    const long long rs = (long long)Ww * ps;                                   // one row down
    const size_t hw = (size_t)HW;
    const int p0 = blockIdx.x * PDF_THREADS * PDF_PPT;
    for (int q = 0; q < PDF_PPT; ++q) {
        const int p = p0 + q * PDF_THREADS + tid;
        if (p >= HW) break;
        const int h = p / Ww, w = p - h * Ww;
        const float* yp = y + ((size_t)row * hw + p) * ps;
        float x[PDF_MAXC];
#pragma unroll
        for (int c = 0; c < PDF_MAXC; ++c) x[c] = c < C ? yp[c] : 0.f;
        float speed = 0.f, vort = 0.f, dvg = 0.f;
        if (DER) {
            const float U = tmg_unnorm_split(yp[0], sc0, sd0, mu0), V = tmg_unnorm_split(yp[1], sc1, sd1, mu1);
            const float uu = U * U, vv = V * V;
            speed = sqrtf(uu + vv);                                        // correctly rounded (hipcc's default for fp32 sqrt)
            if (sten) {
                const bool up = h > 0, dn = h + 1 < Hh, lf = w > 0, rt = w + 1 < Ww;
                const float vx = tmg_sx<false>(yp, ps, rs, 1, sc1, sd1, mu1, up, dn, lf, rt);
                const float uy = tmg_sy<false>(yp, ps, rs, 0, sc0, sd0, mu0, up, dn, lf, rt);
                const float ux = tmg_sx<false>(yp, ps, rs, 0, sc0, sd0, mu0, up, dn, lf, rt);
                const float vy = tmg_sy<false>(yp, ps, rs, 1, sc1, sd1, mu1, up, dn, lf, rt);
                const float t0 = vx * rdx, t1 = uy * rdy, t2 = ux * rdx, t3 = vy * rdy;
                vort = t0 - t1;
                dvg = t2 + t3;
            }
        }
        float d[PDF_MAXF];
        int idx[PDF_MAXF];
#pragma unroll
        for (int f = 0; f < PDF_MAXF; ++f) {
            d[f] = 0.f;
            idx[f] = 0;
            if (f < F) {
                const int kd = a.kind[f];
                float v = kd == 0 ? x[0] : kd == 1 ? x[1] : kd == 2 ? x[2] : kd == 3 ? x[3] : kd == 4 ? speed : kd == 5 ? vort : dvg;
                if (cen && kd < PDF_MAXC) v = v - cen[((size_t)b * C + kd) * hw + p];
                d[f] = v;
                idx[f] = pdf_index(le + f * (nb + 1), nb, ls[f], v);
            }
        }
        int ji[PDF_MAXP];
#pragma unroll
        for (int pr = 0; pr < PDF_MAXP; ++pr) {
            ji[pr] = 0;
            if (pr < P) {
                float va = 0.f, vb = 0.f;
#pragma unroll
                for (int f = 0; f < PDF_MAXF; ++f) {
                    if (f == a.pair[pr][0]) va = d[f];
                    if (f == a.pair[pr][1]) vb = d[f];
                }
                const int ia = pdf_index(lj + (pr * 2) * (nbj + 1), nbj, ls[F + 2 * pr], va);
                const int ib = pdf_index(lj + (pr * 2 + 1) * (nbj + 1), nbj, ls[F + 2 * pr + 1], vb);
                ji[pr] = ia * (nbj + 2) + ib;
            }
        }
#pragma unroll
        for (int r = 0; r < PDF_MAXR; ++r) {
            if (r < R && w >= a.box[r][0] && w < a.box[r][1] && h >= a.box[r][2] && h < a.box[r][3]) {
#pragma unroll
                for (int f = 0; f < PDF_MAXF; ++f)
                    if (f < F) pdf_add(hm + (r * F + f) * (nb + 2), idx[f]);
#pragma unroll
                for (int pr = 0; pr < PDF_MAXP; ++pr)
                    if (pr < P) pdf_add(hj + (r * P + pr) * jb, ji[pr]);
            }
        }
    }
    __syncthreads();
    const bool timed = flags & 1;
    int* sc = step_count + (size_t)b * ocs;
    int* mt = mtime + ((size_t)b * S + m0 + j) * nm;
    for (int i = tid; i < nm; i += PDF_THREADS) {
        const int v = hm[i];
        if (v) {
            atomicAdd(sc + i, v);
            if (timed) atomicAdd(mt + i, v);
        }
    }
    int* sj = step_joint + (size_t)b * jcs;
    int* tj = tjoint + (size_t)b * nj;
    for (int i = tid; i < nj; i += PDF_THREADS) {
        const int v = hj[i];
        if (v) {
            atomicAdd(sj + i, v);
            if (timed) atomicAdd(tj + i, v);
        }
    }
}

extern "C" int tmg_ens_pdf_count(const void* y, const int64_t* y_d, const void* u, const void* mu, const void* sd, const void* center,
                                 const void* edges, const void* jedges, const int64_t* desc, void* step_count, void* step_joint,
                                 void* member_time_count, void* time_joint, const int64_t* o_d, const int64_t* dims, const float* fl,
                                 hipStream_t st) {
    if (!dims) return -3;
    const int64_t k = dims[0], B = dims[1], H = dims[2], W = dims[3], C = dims[4], S = dims[5], m0 = dims[6], F = dims[7], nb = dims[8],
                  P = dims[9], nbj = dims[10], R = dims[11], flags = dims[12];
    if (C < 2 || C > PDF_MAXC || S < 1 || m0 < 0 || k < 1 || m0 + k > S || flags < 0 || flags > 1) return -1;
    if (F < 1 || F > PDF_MAXF || P < 0 || P > PDF_MAXP || R < 1 || R > PDF_MAXR) return -1;
    if (y_d && (y_d[0] < C || y_d[1] < 0 || y_d[1] + C > y_d[0])) return -1;
    PdfArgs a;
    int der = 0;
    for (int i = 0; i < PDF_MAXF; ++i) a.kind[i] = 0;
    for (int i = 0; i < PDF_MAXP; ++i) a.pair[i][0] = a.pair[i][1] = -1;
    for (int i = 0; i < PDF_MAXR; ++i) a.box[i][0] = a.box[i][1] = a.box[i][2] = a.box[i][3] = 0;
    if (desc) {
        for (int64_t f = 0; f < F; ++f) {
            const int64_t kd = desc[f];
            if (kd < 0 || kd > 6 || (kd < PDF_MAXC && kd >= C)) return -1;
            der |= kd >= PDF_MAXC;
            a.kind[f] = (int)kd;
        }
        for (int64_t p = 0; p < P; ++p) {
            const int64_t fi = desc[F + 2 * p], fj = desc[F + 2 * p + 1];
            if (fi < 0 || fi >= F || fj < 0 || fj >= F || fi == fj) return -1;
            a.pair[p][0] = (int)fi;
            a.pair[p][1] = (int)fj;
        }
        for (int64_t r = 0; r < R; ++r) {
            const int64_t* bx = desc + F + 2 * P + 4 * r;
            if (bx[0] < 0 || bx[1] <= bx[0] || bx[1] > W || bx[2] < 0 || bx[3] <= bx[2] || bx[3] > H) return -1;
            for (int i = 0; i < 4; ++i) a.box[r][i] = (int)bx[i];
        }
    }
    const int64_t pd[10] = {k, B, H, W, F, nb, P, nbj, R, der};
    PdfPlan q;
    const int rc = pdf_plan(pd, &q);                                           // its -1, then its -2
    if (rc) return rc;
    if (o_d && (o_d[0] < q.marg || o_d[1] < q.joint)) return -1;
    if (der && fl && (!(fl[0] > 0.f) || !(fl[1] > 0.f) || !(fl[0] <= 3.0e38f) || !(fl[1] <= 3.0e38f))) return -1;
    if (!y_d || !desc || !o_d || (der && !fl)) return -3;
    const int64_t HW = H * W;
    if (y_d[0] >= (1ll << 31) || (k * B) * HW * y_d[0] >= (1ll << 40) || B * C * HW >= (1ll << 40)) return -2;
    if (B * o_d[0] >= (1ll << 40) || B * o_d[1] >= (1ll << 40) || B * S * q.marg >= (1ll << 40)) return -2;
    if (!y || !edges || !step_count || (P && (!jedges || !step_joint))) return -3;
    if (der && (!mu || !sd)) return -3;
    if ((flags & 1) && (!member_time_count || (P && !time_joint))) return -3;
    const float rdx = der ? 0.125f / fl[0] : 0.f, rdy = der ? 0.125f / fl[1] : 0.f;
    dim3 grid((unsigned)q.nsl, (unsigned)(k * B));
    if (der)
        hipLaunchKernelGGL(ens_pdf_count_kernel<1>, grid, dim3(PDF_THREADS), (size_t)q.lds, st, (const float*)y + y_d[1], (int)y_d[0],
                           (const float*)u, (const float*)mu, (const float*)sd, (const float*)center, (const float*)edges,
                           (const float*)jedges, (int*)step_count, (int*)step_joint, (int*)member_time_count, (int*)time_joint,
                           (long long)o_d[0], (long long)o_d[1], (int)B, (int)H, (int)W, (int)C, (int)S, (int)m0, (int)F, (int)nb, (int)P,
                           (int)nbj, (int)R, (int)flags, rdx, rdy, a);
    else
        hipLaunchKernelGGL(ens_pdf_count_kernel<0>, grid, dim3(PDF_THREADS), (size_t)q.lds, st, (const float*)y + y_d[1], (int)y_d[0],
                           (const float*)u, (const float*)mu, (const float*)sd, (const float*)center, (const float*)edges,
                           (const float*)jedges, (int*)step_count, (int*)step_joint, (int*)member_time_count, (int*)time_joint,
                           (long long)o_d[0], (long long)o_d[1], (int)B, (int)H, (int)W, (int)C, (int)S, (int)m0, (int)F, (int)nb, (int)P,
                           (int)nbj, (int)R, (int)flags, rdx, rdy, a);
    TMG_CHECK_LAUNCH();
    return 0;
}
