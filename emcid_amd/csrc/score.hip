// The readout of an edit score (edit_score.EditScorer): what an edit did to the text encoder's own output, reduced on the device.
//   score_rows_kernel    per row pair (a, b) [and a target t]: the sums a relative distance, a cosine and a residual ratio are made
//                        of, optionally behind a LayerNorm of both rows — fp64 from exact conversions of the fp32 inputs
//   score_chains_kernel  per prompt: max / mean / end value of a per-node ratio over the prompt's chain of trie nodes
// Both follow add_layernorm_wave_kernel (attention.hip): one wave per row or prompt, four per workgroup, reductions by shuffles,
// no LDS, no atomics, plain vector loads and stores.  For the SDXL pair of encoders (edit_score.PairEditScorer):
//   score_chains_pair_kernel  score_chains_kernel over the concatenated columns of two encoders, each with a trie of its own
//   score_chains_pair_grid_kernel  score_chains_pair_kernel for every combination of a bank of node sums per encoder (a sweep)
//   score_pooled_kernel       per row pair: the sums the relative distance of text_projection(final_layer_norm(.)) is made of;
//                             four rows per workgroup, normalised once into LDS, for one sweep of the projection matrix
#include "common.h"

// (every product and sum below is rounded on its own: the reference is plain fp64 arithmetic)
#pragma clang fp contract(off)

namespace emcid {

constexpr int SCORE_MAX_V4 = 8;      // float4 chunks per lane: rows of up to 8 * 64 * 4 = 2048 columns

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// What the fp64 LayerNorm of a row pair (a, b) and of its difference takes (the formula below score_rows_kernel's slots), from
// the rows in a wave's registers: the two means and mean(a - b), the two 1 / sqrt(var + eps), and rstd_a - rstd_b.
struct LnPair {
    double ma, mb, dm, ra, rb, dr;
};

__device__ inline LnPair ln_pair_stats(const float4 (&va)[SCORE_MAX_V4], const float4 (&vb)[SCORE_MAX_V4], int lane, int nv, int cols,
                                       double eps) {
    double sa = 0.0, sb = 0.0, sd = 0.0;
#pragma unroll
    for (int i = 0; i < SCORE_MAX_V4; ++i) {
        if (lane + i * 64 < nv) {
            const double ax[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, bx[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sa += ax[k];
                sb += bx[k];
                sd += ax[k] - bx[k];
            }
        }
    }
    const double n = (double)cols;
    const double ma = wave_sum(sa) / n, mb = wave_sum(sb) / n, dm = wave_sum(sd) / n;
    double qa = 0.0, qb = 0.0, qd = 0.0;
#pragma unroll
    for (int i = 0; i < SCORE_MAX_V4; ++i) {
        if (lane + i * 64 < nv) {
            const double ax[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, bx[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double ca = ax[k] - ma, cb = bx[k] - mb, dc = (ax[k] - bx[k]) - dm;
                qa += ca * ca;
                qb += cb * cb;
                qd += dc * (ca + cb);
            }
        }
    }
    const double sda = sqrt(wave_sum(qa) / n + eps), sdb = sqrt(wave_sum(qb) / n + eps);
    return {ma, mb, dm, 1.0 / sda, 1.0 / sdb, -(wave_sum(qd) / n) / (sda * sdb * (sda + sdb))};
}

// out[row][0..7] for row < rows; the row pair lives in registers (as the fp32 values it was loaded as) between the passes.
//   gamma != null: both rows LayerNormed in fp64 — two-pass mean and variance, x^ = (x - mean) rstd gamma + beta — else x^ = x:
//       0: ||a^ - b^||^2    1: ||b^||^2    2: ||a^||^2    3: a^ . b^
//   t != null, on the raw rows:
//       4: ||t - a||^2      5: ||t - b||^2   6: (a - b) . (t - b)
//   7 and every slot not asked for: 0.
// The difference a^ - b^ is never formed from the two normalised rows, whose roundings (1e-16 of |x^|) would be all of it when the
// rows agree to 1e-7: with d = a - b (exact in fp64), ca = a - mean_a, cb = b - mean_b and dm = mean(d)
//       a^ - b^ = gamma [ (d - dm) rstd_a + cb (rstd_a - rstd_b) ]
//       rstd_a - rstd_b = (var_b - var_a) / (sa sb (sa + sb)),  s = sqrt(var + eps),  var_a - var_b = mean((d - dm)(ca + cb))
// every term of which carries the relative error of its own few operations; identical rows give d = 0 in every column and with
// it an exact 0 in slots 0 and 6.
__global__ __launch_bounds__(256) void score_rows_kernel(const float* __restrict__ a, int64_t lda, const float* __restrict__ b,
                                                          int64_t ldb, const float* __restrict__ t, int64_t ldt,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, double eps,
                                                          int rows, int cols, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;       // (whole waves leave: no lane of a wave that stays is missing from the shuffles)
    const int nv = cols / 4;
    const float4* pa = reinterpret_cast<const float4*>(a + row * lda);
    const float4* pb = reinterpret_cast<const float4*>(b + row * ldb);
    float4 va[SCORE_MAX_V4], vb[SCORE_MAX_V4];
#pragma unroll
    for (int i = 0; i < SCORE_MAX_V4; ++i) {
        const int c = lane + i * 64;
        if (c < nv) {
            va[i] = pa[c];
            vb[i] = pb[c];
        }
    }
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (gamma != nullptr) {
        const LnPair ln = ln_pair_stats(va, vb, lane, nv, cols, eps);
        const double ma = ln.ma, mb = ln.mb, dm = ln.dm, ra = ln.ra, rb = ln.rb, dr = ln.dr;
        const float4* pg = reinterpret_cast<const float4*>(gamma);
        const float4* pe = reinterpret_cast<const float4*>(beta);
#pragma unroll
        for (int i = 0; i < SCORE_MAX_V4; ++i) {
            const int c = lane + i * 64;
            if (c < nv) {
                const float4 g4 = pg[c], e4 = pe[c];
                const double ax[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, bx[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
                const double g[4] = {g4.x, g4.y, g4.z, g4.w}, e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double ca = ax[k] - ma, cb = bx[k] - mb, dc = (ax[k] - bx[k]) - dm;
                    const double ah = ca * ra * g[k] + e[k], bh = cb * rb * g[k] + e[k];
                    const double dh = g[k] * (dc * ra + cb * dr);
                    s[0] += dh * dh;
                    s[1] += bh * bh;
                    s[2] += ah * ah;
                    s[3] += ah * bh;
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < SCORE_MAX_V4; ++i) {
            if (lane + i * 64 < nv) {
                const double ax[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, bx[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double d = ax[k] - bx[k];
                    s[0] += d * d;
                    s[1] += bx[k] * bx[k];
                    s[2] += ax[k] * ax[k];
                    s[3] += ax[k] * bx[k];
                }
            }
        }
    }
    if (t != nullptr) {
        const float4* pt = reinterpret_cast<const float4*>(t + row * ldt);
#pragma unroll
        for (int i = 0; i < SCORE_MAX_V4; ++i) {
            const int c = lane + i * 64;
            if (c < nv) {
                const float4 t4 = pt[c];
                const double ax[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, bx[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
                const double tx[4] = {t4.x, t4.y, t4.z, t4.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double ta = tx[k] - ax[k], tb = tx[k] - bx[k];
                    s[4] += ta * ta;
                    s[5] += tb * tb;
                    s[6] += (ax[k] - bx[k]) * tb;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0) {
        double2* o = reinterpret_cast<double2*>(out + row * 8);
        o[0] = make_double2(s[0], s[1]);
        o[1] = make_double2(s[2], s[3]);
        o[2] = make_double2(s[4], s[5]);
        o[3] = make_double2(s[6], 0.0);
    }
}

// ---- one prompt's chain, reduced by one wave: the pieces the three chain kernels below are made of --------------------------------
// A lane takes the chain positions lane and lane + 64.  Every index is checked before the load it is used in.

__device__ __forceinline__ bool in_range(int64_t i, int64_t n) { return i >= 0 && i < n; }

// The admission of one chain: its length depth[e] + 1 if 1 <= n <= 128 and n <= ld_anc, else 0.  ``e_ok``: e is a node of the
// trie (depth[e] is not read otherwise).
__device__ __forceinline__ int chain_admit(bool e_ok, int64_t e, const int32_t* __restrict__ depth, int64_t ld_anc) {
    const int n = e_ok ? depth[e] + 1 : 0;
    return (n >= 1 && n <= 128 && n <= ld_anc) ? n : 0;
}

// The lane's two entries u[j] of the admitted chain anc[e][0 .. n) (n = 0: nothing is read); false when one lies outside [0, U).
__device__ __forceinline__ bool chain_entries(const int32_t* __restrict__ anc, int64_t e, int64_t ld_anc, int64_t U, int n, int lane,
                                              int64_t (&u)[2]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        u[j] = 0;
        if (lane + 64 * j < n) {
            u[j] = anc[e * ld_anc + lane + 64 * j];
            ok = ok && in_range(u[j], U);
        }
    }
    return ok;
}

__device__ __forceinline__ double chain_ratio(double num, double den) { return (num == 0.0 && den == 0.0) ? 0.0 : sqrt(num / den); }

struct ChainAcc {
    double best, sum, last;
    int best_pos;
};

// The lane's share of a chain of n nodes: sums(j) = (num, den) of position lane + 64 j, asked for where take[j].
template <class Sums>
__device__ __forceinline__ ChainAcc chain_lane(const bool (&take)[2], int lane, int n, Sums sums) {
    ChainAcc a = {-1.0, 0.0, 0.0, 1 << 30};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int pos = lane + 64 * j;
        if (take[j]) {
            const double2 s = sums(j);
            const double r = chain_ratio(s.x, s.y);
            a.sum += r;
            if (r > a.best) {         // (positions ascend within a lane: an equal later value does not replace)
                a.best = r;
                a.best_pos = pos;
            }
            if (pos == n - 1) a.last = r;
        }
    }
    return a;
}

// The 64 lanes' shares into every lane: the sum, the end value (one lane holds it, the others 0), the max at its first position.
__device__ __forceinline__ void chain_wave(ChainAcc& a) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a.sum += __shfl_xor(a.sum, o, 64);
        a.last += __shfl_xor(a.last, o, 64);
        const double ob = __shfl_xor(a.best, o, 64);
        const int op = __shfl_xor(a.best_pos, o, 64);
        if (ob > a.best || (ob == a.best && op < a.best_pos)) {
            a.best = ob;
            a.best_pos = op;
        }
    }
}

// Lane 0 writes out4[0..3] = {max, mean, end value, position of the max}, or four NaN for a refused prompt.
__device__ __forceinline__ void chain_write(double* __restrict__ out4, int lane, bool bad, const ChainAcc& a, int n) {
    if (lane != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double2* o = reinterpret_cast<double2*>(out4);
    o[0] = bad ? make_double2(nan, nan) : make_double2(a.best, a.sum / (double)n);
    o[1] = bad ? make_double2(nan, nan) : make_double2(a.last, (double)a.best_pos);
}

// out[p][0..3] = {max, mean, value at the end node, chain position of the max (the first one on a tie)} of
// r(u) = sqrt(node[u][0] / node[u][1]) (0 when both sums are 0) over the chain anc[e][0 .. depth[e]] of e = end_node[p].
// An end node outside [0, U), a chain longer than 128 or than ld_anc, or a chain entry outside [0, U) reads nothing more: the
// prompt's four outputs are NaN.
__global__ __launch_bounds__(256) void score_chains_kernel(const double* __restrict__ node, int64_t U, const int32_t* __restrict__ anc,
                                                            int64_t ld_anc, const int32_t* __restrict__ depth,
                                                            const int64_t* __restrict__ end_node, int B, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= B) return;       // (whole waves leave)
    const int64_t e = end_node[p];
    const int n = chain_admit(in_range(e, U), e, depth, ld_anc);
    int64_t u[2];
    const bool ok = chain_entries(anc, e, ld_anc, U, n, lane, u) && n >= 1;
    bool take[2];
    double2 v[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        take[j] = ok && lane + 64 * j < n;
        if (take[j]) v[j] = *reinterpret_cast<const double2*>(node + u[j] * 8);
    }
    ChainAcc a = chain_lane(take, lane, n, [&](int j) { return v[j]; });
    const int bad = __any(!ok);
    chain_wave(a);
    chain_write(out + (int64_t)p * 4, lane, bad, a, n);
}

// score_chains_kernel over the columns of TWO encoders (an SDXL UNet is conditioned on the concatenation of their token states):
// out[p][0..3] as there, of r_j = sqrt((node1[c1[j]][0] + node2[c2[j]][0]) / (node1[c1[j]][1] + node2[c2[j]][1])) (0 when both
// sums are 0) over position j of the chains c_e = anc_e[end_e[p]][0 .. depth_e[end_e[p]]] in two independently numbered tries.
// Chains of different lengths, and whatever score_chains_kernel refuses in either trie, read nothing more and give four NaN.
__global__ __launch_bounds__(256) void score_chains_pair_kernel(const double* __restrict__ node1, int64_t U1, const int32_t* __restrict__ anc1,
                                                                 int64_t ld_anc1, const int32_t* __restrict__ depth1,
                                                                 const int64_t* __restrict__ end1, const double* __restrict__ node2,
                                                                 int64_t U2, const int32_t* __restrict__ anc2, int64_t ld_anc2,
                                                                 const int32_t* __restrict__ depth2, const int64_t* __restrict__ end2,
                                                                 int B, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= B) return;
    const int64_t e1 = end1[p], e2 = end2[p];
    const bool e_ok = in_range(e1, U1) && in_range(e2, U2);
    const int na = chain_admit(e_ok, e1, depth1, ld_anc1), nb = chain_admit(e_ok, e2, depth2, ld_anc2);
    const int n = na == nb ? na : 0;
    int64_t u1[2], u2[2];
    const bool ok1 = chain_entries(anc1, e1, ld_anc1, U1, n, lane, u1), ok2 = chain_entries(anc2, e2, ld_anc2, U2, n, lane, u2);
    const bool ok = ok1 && ok2 && n >= 1;
    bool take[2];
    double2 v1[2], v2[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        take[j] = ok && lane + 64 * j < n;
        if (take[j]) {
            v1[j] = *reinterpret_cast<const double2*>(node1 + u1[j] * 8);
            v2[j] = *reinterpret_cast<const double2*>(node2 + u2[j] * 8);
        }
    }
    ChainAcc a = chain_lane(take, lane, n, [&](int j) { return make_double2(v1[j].x + v2[j].x, v1[j].y + v2[j].y); });
    const int bad = __any(!ok);
    chain_wave(a);
    chain_write(out + (int64_t)p * 4, lane, bad, a, n);
}

constexpr int GRID_CHUNK = 16;       // combinations per blockIdx.y of score_chains_pair_grid_kernel
constexpr int GRID_FLIGHT = 4;       // of them, those whose node sums are all loaded before the first is reduced

// score_chains_pair_kernel for every combination c < C of a point of encoder 1 with a point of encoder 2 (a sweep over the pair,
// emcid_main.sweep_emcid_sdxl_text_encoders): node_e is a BANK [G_e][U_e][8] of score_rows outputs, combo [C][2] names a bank
// entry of each, and out[c][p][0..3] is what score_chains_pair_kernel writes for prompt p on those two entries — the same bits,
// because both reduce through chain_lane, chain_wave and chain_write.  One wave per prompt, four per workgroup; the prompt's two
// chains are read ONCE into registers (two indices per lane and trie) and judged once, then the wave walks blockIdx.y's chunks of
// GRID_CHUNK combinations, GRID_FLIGHT at a time: their loads are all issued before the first reduction.  A prompt
// score_chains_pair_kernel refuses gets four NaN in every combination, a combination with an entry outside [0, G1) x [0, G2)
// four NaN for every prompt.
__global__ __launch_bounds__(256) void score_chains_pair_grid_kernel(
    const double* __restrict__ node1, int64_t G1, int64_t U1, const int32_t* __restrict__ anc1, int64_t ld_anc1,
    const int32_t* __restrict__ depth1, const int64_t* __restrict__ end1, const double* __restrict__ node2, int64_t G2, int64_t U2,
    const int32_t* __restrict__ anc2, int64_t ld_anc2, const int32_t* __restrict__ depth2, const int64_t* __restrict__ end2, int B,
    const int32_t* __restrict__ combo, int64_t C, double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= B) return;
    const int64_t e1 = end1[p], e2 = end2[p];
    const bool e_ok = in_range(e1, U1) && in_range(e2, U2);
    const int na = chain_admit(e_ok, e1, depth1, ld_anc1), nb = chain_admit(e_ok, e2, depth2, ld_anc2);
    const int n = na == nb ? na : 0;
    int64_t u1[2], u2[2];        // the lane's two chain positions in each trie
    const bool ok1 = chain_entries(anc1, e1, ld_anc1, U1, n, lane, u1), ok2 = chain_entries(anc2, e2, ld_anc2, U2, n, lane, u2);
    const bool ok = ok1 && ok2 && n >= 1;
    const bool take[2] = {ok && lane < n, ok && lane + 64 < n};
    const int bad = __any(!ok);
    const ChainAcc none = {};
    const int64_t n_chunks = (C + GRID_CHUNK - 1) / GRID_CHUNK;
    for (int64_t chunk = blockIdx.y; chunk < n_chunks; chunk += gridDim.y) {
        const int64_t c_end = (chunk + 1) * GRID_CHUNK < C ? (chunk + 1) * GRID_CHUNK : C;
        for (int64_t c0 = chunk * GRID_CHUNK; c0 < c_end; c0 += GRID_FLIGHT) {
            double2 v1[GRID_FLIGHT][2], v2[GRID_FLIGHT][2];
            bool live[GRID_FLIGHT];        // (the same in every lane: the combination's entries and the prompt's verdict)
#pragma unroll
            for (int k = 0; k < GRID_FLIGHT; ++k) {
                live[k] = false;
                if (c0 + k < c_end) {
                    const int64_t g1 = combo[2 * (c0 + k)], g2 = combo[2 * (c0 + k) + 1];
                    live[k] = !bad && in_range(g1, G1) && in_range(g2, G2);
                    if (live[k]) {
                        const double* b1 = node1 + g1 * U1 * 8;
                        const double* b2 = node2 + g2 * U2 * 8;
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            if (take[j]) {
                                v1[k][j] = *reinterpret_cast<const double2*>(b1 + u1[j] * 8);
                                v2[k][j] = *reinterpret_cast<const double2*>(b2 + u2[j] * 8);
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < GRID_FLIGHT; ++k) {
                if (c0 + k >= c_end) break;
                double* o = out + ((c0 + k) * B + p) * 4;
                if (!live[k]) {
                    chain_write(o, lane, true, none, n);
                    continue;
                }
                ChainAcc a = chain_lane(take, lane, n, [&](int j) { return make_double2(v1[k][j].x + v2[k][j].x, v1[k][j].y + v2[k][j].y); });
                chain_wave(a);
                chain_write(o, lane, false, a, n);
            }
        }
    }
}

constexpr int POOLED_ROWS = 4;       // rows per workgroup: all four per sweep of P
constexpr int POOLED_WAVES = 8;      // waves per workgroup: the first four normalise a row each, all eight sweep P

// a lane's chunks of row j of P (zeros behind the last row)
__device__ inline void pooled_load_row(float4 (&p)[SCORE_MAX_V4], const float* __restrict__ P, int64_t ldp, int j, int proj, int lane,
                                       int nv) {
    const float4* pp = reinterpret_cast<const float4*>(P + (int64_t)j * ldp);
#pragma unroll
    for (int i = 0; i < SCORE_MAX_V4; ++i) p[i] = (j < proj && lane + i * 64 < nv) ? pp[lane + i * 64] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// 8 sums over the 64 lanes by a butterfly that halves the number of values at each of its first three steps — the upper half of
// a span keeps the upper half of the values and sends the other half across — (11 shuffles, not 48): value 2 g + k ends on the
// lanes 16 g + 8 k .. 16 g + 8 k + 7, and every lane of 16 g .. 16 g + 15 returns u = value 2 g and v = value 2 g + 1.
__device__ inline void pooled_reduce(const double (&acc)[2 * POOLED_ROWS], int lane, double& u, double& v) {
    const bool h32 = (lane & 32) != 0, h16 = (lane & 16) != 0, h8 = (lane & 8) != 0;
    double r4[4], r2[2];
#pragma unroll
    for (int k = 0; k < 4; ++k) r4[k] = (h32 ? acc[k + 4] : acc[k]) + __shfl_xor(h32 ? acc[k] : acc[k + 4], 32, 64);
#pragma unroll
    for (int k = 0; k < 2; ++k) r2[k] = (h16 ? r4[k + 2] : r4[k]) + __shfl_xor(h16 ? r4[k] : r4[k + 2], 16, 64);
    double r = (h8 ? r2[1] : r2[0]) + __shfl_xor(h8 ? r2[0] : r2[1], 8, 64);
    r += __shfl_xor(r, 4, 64);
    r += __shfl_xor(r, 2, 64);
    r += __shfl_xor(r, 1, 64);
    const double other = __shfl_xor(r, 8, 64);
    u = h8 ? other : r;
    v = h8 ? r : other;
}

// out[row][0..3] = ||P d^||^2, ||P b^||^2, ||P a^||^2, (P a^) . (P b^) with a^, b^ the fp64 LayerNorm of rows a, b and
// d^ = a^ - b^ by score_rows_kernel's formula (from a - b, never from the two normalised rows); P a^ is taken as P d^ + P b^.
// A workgroup of eight waves takes four rows.  Waves 0-3 normalise one each and leave d^ and b^ in LDS as fp64 — eight vectors,
// each as two planes of double2 ((x0, x1) and (x2, x3) of a lane's float4 chunk), so that a lane reads 16 contiguous bytes beside
// its neighbour's.  Then every wave takes pairs of rows of P: its chunks of both in registers (the next pair's loads in flight),
// eight partial dot products per lane and row of P, reduced by pooled_reduce, which leaves P[j] . d^ and P[j] . b^ of row g on
// the lanes 16 g .. 16 g + 15.  The waves' sums over their rows of P meet in LDS and are added in wave order: every sum has one
// fixed order.
__global__ __launch_bounds__(64 * POOLED_WAVES) void score_pooled_kernel(
    const float* __restrict__ a, int64_t lda, const float* __restrict__ b, int64_t ldb, const float* __restrict__ gamma,
    const float* __restrict__ beta, double eps, const float* __restrict__ P, int64_t ldp, int rows, int cols, int proj,
    double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double2 pooled_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nv = cols / 4;
    const int64_t base = (int64_t)blockIdx.x * POOLED_ROWS;
    // vector v = 2 g + (0: d^, 1: b^) of row base + g, plane q, chunk c: pooled_lds[(2 v + q) nv + c]
    if (wave < POOLED_ROWS) {
        const int64_t row = base + wave;
        double2* vd = pooled_lds + (size_t)(4 * wave) * nv;
        double2* vb_ = vd + 2 * (size_t)nv;
        if (row < rows) {
            const float4* pa = reinterpret_cast<const float4*>(a + row * lda);
            const float4* pb = reinterpret_cast<const float4*>(b + row * ldb);
            float4 va[SCORE_MAX_V4], vb[SCORE_MAX_V4];
#pragma unroll
            for (int i = 0; i < SCORE_MAX_V4; ++i) {
                const int c = lane + i * 64;
                if (c < nv) {
                    va[i] = pa[c];
                    vb[i] = pb[c];
                }
            }
            const LnPair ln = ln_pair_stats(va, vb, lane, nv, cols, eps);
            const float4* pg = reinterpret_cast<const float4*>(gamma);
            const float4* pe = reinterpret_cast<const float4*>(beta);
#pragma unroll
            for (int i = 0; i < SCORE_MAX_V4; ++i) {
                const int c = lane + i * 64;
                if (c < nv) {
                    const float4 g4 = pg[c], e4 = pe[c];
                    const double ax[4] = {va[i].x, va[i].y, va[i].z, va[i].w}, bx[4] = {vb[i].x, vb[i].y, vb[i].z, vb[i].w};
                    const double g[4] = {g4.x, g4.y, g4.z, g4.w}, e[4] = {e4.x, e4.y, e4.z, e4.w};
                    double dh[4], bh[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const double cb = bx[k] - ln.mb, dc = (ax[k] - bx[k]) - ln.dm;
                        bh[k] = cb * ln.rb * g[k] + e[k];
                        dh[k] = g[k] * (dc * ln.ra + cb * ln.dr);
                    }
                    vd[c] = make_double2(dh[0], dh[1]);
                    vd[nv + c] = make_double2(dh[2], dh[3]);
                    vb_[c] = make_double2(bh[0], bh[1]);
                    vb_[nv + c] = make_double2(bh[2], bh[3]);
                }
            }
        } else {          // (behind the last row: zeros, so that the sweep has no branch per row; nothing of them is stored)
            for (int c = lane; c < 4 * nv; c += 64) vd[c] = make_double2(0.0, 0.0);
        }
    }
    __syncthreads();
    // wave w takes the PAIRS of rows (2 t, 2 t + 1) of P, t = w, w + 8, ...: one read of the eight vectors serves both rows, and
    // the two butterflies are independent chains.  A row behind the last one is zeros: its dot products add an exact 0.
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const int n_pairs = (proj + 1) / 2;
    float4 pn0[SCORE_MAX_V4], pn1[SCORE_MAX_V4];
    if (wave < n_pairs) {
        pooled_load_row(pn0, P, ldp, 2 * wave, proj, lane, nv);
        pooled_load_row(pn1, P, ldp, 2 * wave + 1, proj, lane, nv);
    }
    for (int t = wave; t < n_pairs; t += POOLED_WAVES) {
        float4 pc0[SCORE_MAX_V4], pc1[SCORE_MAX_V4];
#pragma unroll
        for (int i = 0; i < SCORE_MAX_V4; ++i) {
            pc0[i] = pn0[i];
            pc1[i] = pn1[i];
        }
        if (t + POOLED_WAVES < n_pairs) {       // (the next pair's loads are in flight under this pair's products)
            pooled_load_row(pn0, P, ldp, 2 * (t + POOLED_WAVES), proj, lane, nv);
            pooled_load_row(pn1, P, ldp, 2 * (t + POOLED_WAVES) + 1, proj, lane, nv);
        }
        double acc0[2 * POOLED_ROWS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, acc1[2 * POOLED_ROWS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        {
            // (the dot products may fuse: a fused multiply-add rounds once, and the order of the terms stays as written)
#pragma clang fp contract(fast)
#pragma unroll
            for (int i = 0; i < SCORE_MAX_V4; ++i) {
                const int c = lane + i * 64;
                if (c < nv) {
                    const double p0[4] = {pc0[i].x, pc0[i].y, pc0[i].z, pc0[i].w}, p1[4] = {pc1[i].x, pc1[i].y, pc1[i].z, pc1[i].w};
#pragma unroll
                    for (int v = 0; v < 2 * POOLED_ROWS; ++v) {
                        const double2 lo = pooled_lds[(size_t)(2 * v) * nv + c], hi = pooled_lds[(size_t)(2 * v + 1) * nv + c];
                        acc0[v] += p0[0] * lo.x;
                        acc1[v] += p1[0] * lo.x;
                        acc0[v] += p0[1] * lo.y;
                        acc1[v] += p1[1] * lo.y;
                        acc0[v] += p0[2] * hi.x;
                        acc1[v] += p1[2] * hi.x;
                        acc0[v] += p0[3] * hi.y;
                        acc1[v] += p1[3] * hi.y;
                    }
                }
            }
        }
        double u0, v0, u1, v1;
        pooled_reduce(acc0, lane, u0, v0);
        pooled_reduce(acc1, lane, u1, v1);
        const double w0 = u0 + v0, w1 = u1 + v1;
        s[0] += u0 * u0;
        s[1] += v0 * v0;
        s[2] += w0 * w0;
        s[3] += w0 * v0;
        s[0] += u1 * u1;
        s[1] += v1 * v1;
        s[2] += w1 * w1;
        s[3] += w1 * v1;
    }
    double* part = reinterpret_cast<double*>(pooled_lds + (size_t)(4 * POOLED_ROWS) * nv);      // [wave][row][4]
    if ((lane & 15) == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) part[(wave * POOLED_ROWS + (lane >> 4)) * 4 + k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < POOLED_ROWS * 4) {
        const int g = threadIdx.x >> 2;
        if (base + g < rows) {
            double t = part[threadIdx.x];
#pragma unroll
            for (int wv = 1; wv < POOLED_WAVES; ++wv) t += part[wv * POOLED_ROWS * 4 + threadIdx.x];
            out[(base + g) * 4 + (threadIdx.x & 3)] = t;
        }
    }
}

}  // namespace emcid

using namespace emcid;

extern "C" {

int emcid_score_rows_f32(const float* a, int64_t lda, const float* b, int64_t ldb, const float* t, int64_t ldt, const float* gamma,
                         const float* beta, float eps, int64_t rows, int64_t cols, double* out, void* stream) {
    EMCID_CHECK_ARG(a && b && out && rows > 0 && rows < (1LL << 31) && cols > 0);
    EMCID_CHECK_ARG(cols % 4 == 0 && cols <= SCORE_MAX_V4 * 64 * 4);
    EMCID_CHECK_ARG(lda % 4 == 0 && ldb % 4 == 0 && lda >= cols && ldb >= cols && (t == nullptr || (ldt % 4 == 0 && ldt >= cols)));
    EMCID_CHECK_ARG((gamma == nullptr) == (beta == nullptr));
    EMCID_CHECK_ARG(aligned16(a) && aligned16(b) && aligned16(t) && aligned16(gamma) && aligned16(beta) && aligned16(out));
    ScopedProf sp(KC_MISC, (hipStream_t)stream);
    hipLaunchKernelGGL(score_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, a, lda, b, ldb, t, ldt,
                       gamma, beta, (double)eps, (int)rows, (int)cols, out);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int emcid_score_chains_f64(const double* node, int64_t U, const int32_t* anc, int64_t ld_anc, const int32_t* depth,
                           const int64_t* end_node, int64_t B, double* out, void* stream) {
    EMCID_CHECK_ARG(node && anc && depth && end_node && out && U > 0 && U < (1LL << 31) && ld_anc > 0 && B > 0 && B < (1LL << 31));
    EMCID_CHECK_ARG(aligned16(node) && aligned16(out));
    ScopedProf sp(KC_MISC, (hipStream_t)stream);
    hipLaunchKernelGGL(score_chains_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, node, U, anc, ld_anc,
                       depth, end_node, (int)B, out);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int emcid_score_chains_pair_f64(const double* node1, int64_t U1, const int32_t* anc1, int64_t ld_anc1, const int32_t* depth1,
                                const int64_t* end1, const double* node2, int64_t U2, const int32_t* anc2, int64_t ld_anc2,
                                const int32_t* depth2, const int64_t* end2, int64_t B, double* out, void* stream) {
    EMCID_CHECK_ARG(node1 && anc1 && depth1 && end1 && node2 && anc2 && depth2 && end2 && out);
    EMCID_CHECK_ARG(U1 > 0 && U1 < (1LL << 31) && U2 > 0 && U2 < (1LL << 31) && ld_anc1 > 0 && ld_anc2 > 0 && B > 0 && B < (1LL << 31));
    EMCID_CHECK_ARG(aligned16(node1) && aligned16(node2) && aligned16(out));
    ScopedProf sp(KC_MISC, (hipStream_t)stream);
    hipLaunchKernelGGL(score_chains_pair_kernel, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, node1, U1, anc1,
                       ld_anc1, depth1, end1, node2, U2, anc2, ld_anc2, depth2, end2, (int)B, out);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int emcid_score_chains_pair_grid_f64(const double* node1, int64_t G1, int64_t U1, const int32_t* anc1, int64_t ld_anc1,
                                     const int32_t* depth1, const int64_t* end1, const double* node2, int64_t G2, int64_t U2,
                                     const int32_t* anc2, int64_t ld_anc2, const int32_t* depth2, const int64_t* end2, int64_t B,
                                     const int32_t* combo, int64_t C, double* out, void* stream) {
    EMCID_CHECK_ARG(node1 && anc1 && depth1 && end1 && node2 && anc2 && depth2 && end2 && combo && out);
    EMCID_CHECK_ARG(G1 > 0 && G1 < (1LL << 31) && G2 > 0 && G2 < (1LL << 31) && C > 0 && C < (1LL << 31));
    EMCID_CHECK_ARG(U1 > 0 && U1 < (1LL << 31) && U2 > 0 && U2 < (1LL << 31) && ld_anc1 > 0 && ld_anc2 > 0 && B > 0 && B < (1LL << 31));
    // (the kernel's offsets are 64-bit: a bank of G U 8 doubles and the C B 4 outputs must be addressable)
    EMCID_CHECK_ARG(G1 <= (1LL << 58) / U1 && G2 <= (1LL << 58) / U2 && C <= (1LL << 58) / B);
    EMCID_CHECK_ARG(aligned16(node1) && aligned16(node2) && aligned16(out));
    const int64_t n_chunks = (C + GRID_CHUNK - 1) / GRID_CHUNK;
    ScopedProf sp(KC_MISC, (hipStream_t)stream);
    hipLaunchKernelGGL(score_chains_pair_grid_kernel, dim3((unsigned)((B + 3) / 4), (unsigned)(n_chunks < 65535 ? n_chunks : 65535)),
                       dim3(256), 0, (hipStream_t)stream, node1, G1, U1, anc1, ld_anc1, depth1, end1, node2, G2, U2, anc2, ld_anc2,
                       depth2, end2, (int)B, combo, C, out);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

int emcid_score_pooled_f32(const float* a, int64_t lda, const float* b, int64_t ldb, const float* gamma, const float* beta, float eps,
                           const float* P, int64_t ldp, int64_t rows, int64_t cols, int64_t proj, double* out, void* stream) {
    EMCID_CHECK_ARG(a && b && gamma && beta && P && out && rows > 0 && rows < (1LL << 31) && cols > 0 && proj >= 1 && proj < (1LL << 31));
    EMCID_CHECK_ARG(cols % 4 == 0 && cols <= SCORE_MAX_V4 * 64 * 4);
    EMCID_CHECK_ARG(lda % 4 == 0 && ldb % 4 == 0 && ldp % 4 == 0 && lda >= cols && ldb >= cols && ldp >= cols);
    EMCID_CHECK_ARG(aligned16(a) && aligned16(b) && aligned16(gamma) && aligned16(beta) && aligned16(P) && aligned16(out));
    // eight fp64 vectors of cols entries and the waves' 8 x 4 x 4 partial sums: 129 KiB at cols = 2048
    const size_t lds = (size_t)cols * 2 * POOLED_ROWS * sizeof(double) + POOLED_WAVES * POOLED_ROWS * 4 * sizeof(double);
    if (lds > 64 * 1024) {
        static bool attr_set[64] = {};      // a function attribute is per device
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (dev < 0 || dev >= 64 || !attr_set[dev]) {
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&score_pooled_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    160 * 1024) != hipSuccess)
                return fail(EMCID_ERR_HIP, __func__, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
            if (dev >= 0 && dev < 64) attr_set[dev] = true;
        }
    }
    ScopedProf sp(KC_MISC, (hipStream_t)stream);
    hipLaunchKernelGGL(score_pooled_kernel, dim3((unsigned)((rows + POOLED_ROWS - 1) / POOLED_ROWS)), dim3(64 * POOLED_WAVES), lds,
                       (hipStream_t)stream, a, lda, b, ldb, gamma, beta, (double)eps, P, ldp, (int)rows, (int)cols, (int)proj, out);
    EMCID_CHECK_LAUNCH();
    return EMCID_OK;
}

}  // extern "C"
