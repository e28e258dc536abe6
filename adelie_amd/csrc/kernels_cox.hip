// kernels_cox.hip — the Cox proportional-hazards family (reference glm_cox.ipp:356-514, 649-748) on the device.
//
// Unlike every other family the gradient and Hessian at row i are sums over risk sets, so one evaluation is a chain of
// stratum-segmented scans, gathers and tie-group sums over n (all in f64, whatever the design's dtype):
//   K1 cox_max          c = max eta (block partials; each consumer block folds them itself)
//   K2 cox_scan1_up     z = w exp(eta - c) gathered into stop order and start order; tile aggregates of 3 suffix scans
//   K3 cox_scan1_down   the suffix scans: z by stratum (stop order), z * ind by tie group (stop order), z by stratum (start order)
//   K4 cox_scan2_up     risk totals, v = d wbar / risk, v2 = d wbar / risk^2, the log-risk part of the loss; tile aggregates of
//                       4 prefix scans
//   K5 cox_scan2_down   the prefix scans: v, v2 by stratum; v sigma ind, v2 sigma (2 - sigma) ind by tie group
//   K6 cox_combine      row order: gathers at the precomputed positions -> grad, hess; the -sum w d (eta - c) part of the loss
//   K7 cox_loss_final   one block adds the loss partials in a fixed order
// Scans are reduce-then-scan over tiles of TILE elements with a fixed combination tree (the carry of tile b is folded from
// the aggregates of tiles 0..b-1 by each block itself, no look-back, no atomics): two evaluations of the same input are
// bit-identical.  A segmented sum never crosses a stratum (or tie group) boundary.
// cox_loss_batch (B1-B5 below) is the loss-only form of the chain for many etas under two packs at once: cv_grpnet's fold losses.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "cox.hpp"

namespace ahip {

namespace {

constexpr int CT = 256;          // threads per block
constexpr int CE = 4;            // elements per thread
constexpr int TILE = CT * CE;    // elements per tile (= per block)
constexpr int NW = CT / 64;      // waves per block

__host__ __device__ inline int64_t n_tiles(int64_t n) { return (n + TILE - 1) / TILE; }

// scratch layout (doubles): 6 n-vectors, then per-tile aggregates of both scans, max partials, loss partials, the loss
struct Layout {
    int64_t n, nt;
    __host__ __device__ size_t a(int k) const { return size_t(k) * size_t(n); }
    __host__ __device__ size_t agg1() const { return size_t(6) * size_t(n); }            // nt * 3 sums, nt * 3 flags
    __host__ __device__ size_t agg2() const { return agg1() + size_t(6) * size_t(nt); }  // nt * 4 sums, nt * 4 flags
    __host__ __device__ size_t pmax() const { return agg2() + size_t(8) * size_t(nt); }  // nt
    __host__ __device__ size_t lossp() const { return pmax() + size_t(nt); }            // 2 nt
    __host__ __device__ size_t loss() const { return lossp() + size_t(2) * size_t(nt); }
    __host__ __device__ size_t total() const { return loss() + 1; }
};

// segmented-sum operator on (flag, sum) pairs, A before B: a flag restarts the sum
__device__ __forceinline__ void seg_combine(bool af, double as, bool& bf, double& bs) {
    if (!bf) bs = as + bs;
    bf = af || bf;
}

// Block-wide exclusive segmented scan of the threads' aggregates (thread order), C channels at once; `tf` / `ts` receive the
// block's total.  Fixed tree: Kogge-Stone inside each wave, the wave totals folded in wave order.
template <int C>
__device__ void block_seg_scan(bool (&f)[C], double (&s)[C], bool (&tf)[C], double (&ts)[C]) {
    __shared__ double wsum[NW][C];
    __shared__ int wflag[NW][C];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        bool F = f[c];
        double S = s[c];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const double ps = __shfl_up(S, d, 64);
            const int pf = __shfl_up(int(F), d, 64);
            if (lane >= d) seg_combine(pf != 0, ps, F, S);
        }
        // exclusive: the inclusive value of the previous lane
        double es = __shfl_up(S, 1, 64);
        int ef = __shfl_up(int(F), 1, 64);
        if (lane == 0) { es = 0; ef = 0; }
        if (lane == 63) { wsum[wv][c] = S; wflag[wv][c] = int(F); }
        f[c] = ef != 0;
        s[c] = es;
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c) {
        bool pf = false;
        double ps = 0;
        for (int w = 0; w < wv; ++w) { // prefix of the waves before this one
            bool F = wflag[w][c] != 0;
            double S = wsum[w][c];
            seg_combine(pf, ps, F, S);
            pf = F; ps = S;
        }
        seg_combine(pf, ps, f[c], s[c]);
        bool F = false;
        double S = 0;
        for (int w = 0; w < NW; ++w) {
            bool G = wflag[w][c] != 0;
            double V = wsum[w][c];
            seg_combine(F, S, G, V);
            F = G; S = V;
        }
        tf[c] = F;
        ts[c] = S;
    }
    __syncthreads(); // (the shared arrays may be reused by a later call)
}

// the carry into tile b: the aggregates of tiles 0..b-1 folded in order (each thread a contiguous chunk, then the block)
template <int C>
__device__ void tile_carry(const double* agg, int64_t nt, int64_t b, bool (&cf)[C], double (&cs)[C]) {
    const double* aggf = agg + nt * C;
    const int64_t chunk = (b + CT - 1) / CT;
    const int64_t lo = int64_t(threadIdx.x) * chunk, hi = min(lo + chunk, b);
    bool f[C];
    double s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { f[c] = false; s[c] = 0; }
    for (int64_t t = lo; t < hi; ++t) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            bool F = aggf[t * C + c] != 0;
            double S = agg[t * C + c];
            seg_combine(f[c], s[c], F, S);
            f[c] = F; s[c] = S;
        }
    }
    block_seg_scan<C>(f, s, cf, cs);
}

// c = max eta, folded by every block from the K1 partials
__device__ double fold_max(const double* pmax, int64_t nt) {
    __shared__ double red[NW];
    double m = -INFINITY;
    for (int64_t t = threadIdx.x; t < nt; t += CT) m = fmax(m, pmax[t]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_down(m, d, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) r = fmax(r, red[w]);
    __syncthreads();
    return r;
}

__device__ double block_sum(double v) {
    __shared__ double red[NW];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) r += red[w];
    __syncthreads();
    return r;
}

template <class T>
__global__ __launch_bounds__(CT) void cox_max_kernel(const T* __restrict__ eta, int64_t n, double* __restrict__ pmax) {
    __shared__ double red[NW];
    double m = -INFINITY;
    const int64_t base = int64_t(blockIdx.x) * TILE;
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int64_t i = base + int64_t(e) * CT + threadIdx.x;
        if (i < n) m = fmax(m, double(eta[i]));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_down(m, d, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = red[0];
        for (int w = 1; w < NW; ++w) r = fmax(r, red[w]);
        pmax[blockIdx.x] = r;
    }
}

// Scan 1 (suffix): logical element j is stop / start position q = n - 1 - j; a segment "starts" (logically) at the LAST
// position of a stratum / tie group.  Channels: 0 z by stratum (stop order), 1 z * ind by tie group (stop order), 2 z by
// stratum (start order).
template <class T, bool DOWN>
__global__ __launch_bounds__(CT) void cox_scan1_kernel(CoxPack pk, const T* __restrict__ eta, double* __restrict__ scr) {
    const Layout L{pk.n, n_tiles(pk.n)};
    const int64_t n = pk.n, b = blockIdx.x;
    double* zto = scr + L.a(0);
    double* zso = scr + L.a(1);
    double* agg = scr + L.agg1();
    double v[CE][3];
    bool fl[CE][3];
    if (!DOWN) {
        const double c = fold_max(scr + L.pmax(), L.nt);
#pragma unroll
        for (int e = 0; e < CE; ++e) {
            const int64_t j = b * TILE + int64_t(threadIdx.x) * CE + e;
            if (j < n) {
                const int64_t q = n - 1 - j;
                const int64_t rt = pk.to[q], rs = pk.so[q];
                const double zt = pk.w[rt] * exp(double(eta[rt]) - c);
                const double zs = pk.w[rs] * exp(double(eta[rs]) - c);
                zto[q] = zt;
                zso[q] = zs;
                const uint8_t g = pk.flags[q];
                v[e][0] = zt; v[e][1] = (g & COX_IND) ? zt : 0.0; v[e][2] = zs;
                fl[e][0] = (g & COX_STRATUM_LAST) != 0; fl[e][1] = (g & COX_TIE_LAST) != 0; fl[e][2] = fl[e][0];
            } else {
                v[e][0] = v[e][1] = v[e][2] = 0;
                fl[e][0] = fl[e][1] = fl[e][2] = true;
            }
        }
    } else {
#pragma unroll
        for (int e = 0; e < CE; ++e) {
            const int64_t j = b * TILE + int64_t(threadIdx.x) * CE + e;
            if (j < n) {
                const int64_t q = n - 1 - j;
                const uint8_t g = pk.flags[q];
                const double zt = zto[q];
                v[e][0] = zt; v[e][1] = (g & COX_IND) ? zt : 0.0; v[e][2] = zso[q];
                fl[e][0] = (g & COX_STRATUM_LAST) != 0; fl[e][1] = (g & COX_TIE_LAST) != 0; fl[e][2] = fl[e][0];
            } else {
                v[e][0] = v[e][1] = v[e][2] = 0;
                fl[e][0] = fl[e][1] = fl[e][2] = true;
            }
        }
    }
    // the thread's own aggregate
    bool f[3];
    double s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        f[k] = false; s[k] = 0;
#pragma unroll
        for (int e = 0; e < CE; ++e) {
            bool F = fl[e][k];
            double S = v[e][k];
            seg_combine(f[k], s[k], F, S);
            f[k] = F; s[k] = S;
        }
    }
    bool tf[3];
    double ts[3];
    block_seg_scan<3>(f, s, tf, ts);
    if (!DOWN) {
        if (threadIdx.x < 3) {
            agg[b * 3 + threadIdx.x] = ts[threadIdx.x];
            agg[L.nt * 3 + b * 3 + threadIdx.x] = tf[threadIdx.x] ? 1.0 : 0.0;
        }
        return;
    }
    bool cf[3];
    double cs[3];
    tile_carry<3>(agg, L.nt, b, cf, cs);
    double* out0 = scr + L.a(2);
    double* out1 = scr + L.a(3);
    double* out2 = scr + L.a(4);
#pragma unroll
    for (int k = 0; k < 3; ++k) seg_combine(cf[k], cs[k], f[k], s[k]); // incoming sum of the thread's first element
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int64_t j = b * TILE + int64_t(threadIdx.x) * CE + e;
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = fl[e][k] ? v[e][k] : s[k] + v[e][k];
        if (j < n) {
            const int64_t q = n - 1 - j;
            out0[q] = s[0];
            out1[q] = s[1];
            out2[q] = s[2];
        }
    }
}

// Scan 2 (prefix, stop order).  UP: risk totals, v, v2, the log-risk part of the loss, tile aggregates.  DOWN: the scans.
// Channels: 0 v by stratum, 1 v2 by stratum, 2 v sigma ind by tie group, 3 v2 sigma (2 - sigma) ind by tie group.
template <class T, bool DOWN>
__global__ __launch_bounds__(CT) void cox_scan2_kernel(CoxPack pk, double* __restrict__ scr, double neg_max) {
    const Layout L{pk.n, n_tiles(pk.n)};
    const int64_t n = pk.n, b = blockIdx.x;
    double* vv = scr + L.a(0);
    double* vv2 = scr + L.a(1);
    double* agg = scr + L.agg2();
    double v[CE][4];
    bool fl[CE][4];
    double lsum = 0;
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int64_t q = b * TILE + int64_t(threadIdx.x) * CE + e;
        if (q < n) {
            const uint8_t g = pk.flags[q];
            const double sc = pk.scale[q];
            double a, a2;
            if (!DOWN) {
                const double* s_stop = scr + L.a(2);
                const double* t_tie = scr + L.a(3);
                const double* s_start = scr + L.a(4);
                const int64_t gs = pk.gstart[q], bp = pk.bpos[q];
                const double risk = s_stop[gs] - (bp >= 0 ? s_start[bp] : 0.0);
                const double rt = risk - sc * ((g & COX_IND) ? t_tie[gs] : 0.0);
                const double dw = pk.dw[q];
                a = dw != 0 ? dw / rt : 0.0;
                a2 = dw != 0 ? dw / (rt * rt) : 0.0;
                vv[q] = a;
                vv2[q] = a2;
                if (dw != 0) lsum += dw * fmax(log(fmax(rt, 0.0)), neg_max);
            } else {
                a = vv[q];
                a2 = vv2[q];
            }
            const bool ind = (g & COX_IND) != 0;
            v[e][0] = a; v[e][1] = a2;
            v[e][2] = ind ? a * sc : 0.0; v[e][3] = ind ? a2 * sc * (2 - sc) : 0.0;
            fl[e][0] = fl[e][1] = (g & COX_STRATUM_FIRST) != 0;
            fl[e][2] = fl[e][3] = (g & COX_TIE_FIRST) != 0;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) { v[e][k] = 0; fl[e][k] = true; }
        }
    }
    bool f[4];
    double s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[k] = false; s[k] = 0;
#pragma unroll
        for (int e = 0; e < CE; ++e) {
            bool F = fl[e][k];
            double S = v[e][k];
            seg_combine(f[k], s[k], F, S);
            f[k] = F; s[k] = S;
        }
    }
    bool tf[4];
    double ts[4];
    block_seg_scan<4>(f, s, tf, ts);
    if (!DOWN) {
        lsum = block_sum(lsum);
        if (threadIdx.x < 4) {
            agg[b * 4 + threadIdx.x] = ts[threadIdx.x];
            agg[L.nt * 4 + b * 4 + threadIdx.x] = tf[threadIdx.x] ? 1.0 : 0.0;
        }
        if (threadIdx.x == 0) scr[L.lossp() + b] = lsum;
        return;
    }
    bool cf[4];
    double cs[4];
    tile_carry<4>(agg, L.nt, b, cf, cs);
#pragma unroll
    for (int k = 0; k < 4; ++k) seg_combine(cf[k], cs[k], f[k], s[k]);
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int64_t q = b * TILE + int64_t(threadIdx.x) * CE + e;
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = fl[e][k] ? v[e][k] : s[k] + v[e][k];
        if (q < n) {
#pragma unroll
            for (int k = 0; k < 4; ++k) scr[L.a(2 + k) + q] = s[k];
        }
    }
}

// row order: grad = w d - z (P1[a] - ind G3[a] - P1[b]),  hess = w d - grad - z^2 (P2[a] - ind H3[a] - P2[b])
template <class T>
__global__ __launch_bounds__(CT) void cox_combine_kernel(CoxPack pk, const T* __restrict__ eta, T* __restrict__ grad,
                                                         T* __restrict__ hess, double* __restrict__ scr) {
    const Layout L{pk.n, n_tiles(pk.n)};
    const int64_t n = pk.n, b = blockIdx.x;
    const double c = fold_max(scr + L.pmax(), L.nt);
    const double* P1 = scr + L.a(2);
    const double* P2 = scr + L.a(3);
    const double* G3 = scr + L.a(4);
    const double* H3 = scr + L.a(5);
    double lsum = 0;
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int64_t r = b * TILE + int64_t(e) * CT + threadIdx.x;
        if (r >= n) continue;
        const double er = double(eta[r]) - c;
        const double wd = pk.wd[r];
        lsum -= wd * er;
        if (!grad && !hess) continue;
        const double z = pk.w[r] * exp(er);
        const int64_t ia = pk.row_a[r], ib = pk.row_b[r];
        const double ind = pk.ind[r];
        const double gs = P1[ia] - ind * G3[ia] - (ib >= 0 ? P1[ib] : 0.0);
        const double g = wd - z * gs;
        if (grad) grad[r] = T(g);
        if (hess) {
            const double hs = P2[ia] - ind * H3[ia] - (ib >= 0 ? P2[ib] : 0.0);
            hess[r] = T(wd - g - z * z * hs);
        }
    }
    lsum = block_sum(lsum);
    if (threadIdx.x == 0) scr[L.lossp() + L.nt + b] = lsum;
}

__global__ __launch_bounds__(CT) void cox_loss_final_kernel(double* __restrict__ scr, int64_t n) {
    const Layout L{n, n_tiles(n)};
    const int64_t m = 2 * L.nt;
    const int64_t chunk = (m + CT - 1) / CT;
    double s = 0;
    for (int64_t t = int64_t(threadIdx.x) * chunk; t < min(int64_t(threadIdx.x + 1) * chunk, m); ++t) s += scr[L.lossp() + t];
    s = block_sum(s);
    if (threadIdx.x == 0) scr[L.loss()] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// cox_loss_batch: the loss alone at `lc` etas under two packs over the same rows (cv_grpnet's full-data and training families).
// The chain above with lambda on blockIdx.y and both packs in one kernel body, without scan 2's prefix scans:
//   B1 cox_batch_max         c_l = max eta_l (one maximum per lambda; it does not depend on the weights)
//   B2 cox_batch_scan1_up    K2 for both packs: eta is gathered and exp(eta - c_l) taken once where the packs name the same row
//   B3 cox_batch_scan1_down  K3 for both packs, in place (a thread reads its own z before it writes the sums over them)
//   B4 cox_batch_loss_parts  the loss halves of K4 (log-risk, stop order) and K6 (-sum w d (eta - c), row order)
//   B5 cox_batch_loss_final  K7 per (lambda, pack)
// Every sum runs over the same tiles through the same trees as in cox_eval (thread_fold = the loops of K2 / K3, block_seg_scan,
// tile_carry, block_sum, the chunked final fold over "log-risk partials, then row partials"), so the losses are cox_eval's bits.
// Each pack's own index arrays are read: nothing assumes that two cox_create calls sorted alike.

// scratch layout (doubles): per (lambda, pack) 3 n-vectors, then per (lambda, pack) the scan-1 tile aggregates, per lambda the
// max partials, per (lambda, pack) the loss partials
struct BatchLayout {
    int64_t n, nt, lc;
    __host__ __device__ size_t lf(int64_t l, int f) const { return size_t(l) * 2 + size_t(f); }
    __host__ __device__ size_t vec(int64_t l, int f, int k) const { return (lf(l, f) * 3 + size_t(k)) * size_t(n); } // z_to -> S_stop, z_so -> S_start, T_tie
    __host__ __device__ size_t agg0() const { return size_t(6) * size_t(lc) * size_t(n); }
    __host__ __device__ size_t agg(int64_t l, int f) const { return agg0() + lf(l, f) * 6 * size_t(nt); }   // nt * 3 sums, nt * 3 flags
    __host__ __device__ size_t pmax(int64_t l) const { return agg0() + (size_t(12) * size_t(lc) + size_t(l)) * size_t(nt); }
    __host__ __device__ size_t lossp(int64_t l, int f) const { return agg0() + (size_t(13) * size_t(lc) + lf(l, f) * 2) * size_t(nt); } // 2 nt
    __host__ __device__ size_t total() const { return agg0() + size_t(17) * size_t(lc) * size_t(nt); }
};

// eta_l at row i, formed in T in the order glm_loss2_kernel forms it
template <class T>
__device__ __forceinline__ T batch_eta(const T* __restrict__ bl, T b0, const T* __restrict__ off, int64_t i) {
    return bl[i] + b0 + off[i];
}

// a thread's aggregate of its CE consecutive elements
template <int C>
__device__ __forceinline__ void thread_fold(const double (&v)[CE][C], const bool (&fl)[CE][C], bool (&f)[C], double (&s)[C]) {
#pragma unroll
    for (int k = 0; k < C; ++k) {
        f[k] = false; s[k] = 0;
#pragma unroll
        for (int e = 0; e < CE; ++e) {
            bool F = fl[e][k];
            double S = v[e][k];
            seg_combine(f[k], s[k], F, S);
            f[k] = F; s[k] = S;
        }
    }
}

// scan 1's three channels of one element from its z values and flags (as K2 / K3 fill them)
__device__ __forceinline__ void scan1_channels(uint8_t g, double zt, double zs, double (&v)[3], bool (&fl)[3]) {
    v[0] = zt; v[1] = (g & COX_IND) ? zt : 0.0; v[2] = zs;
    fl[0] = (g & COX_STRATUM_LAST) != 0; fl[1] = (g & COX_TIE_LAST) != 0; fl[2] = fl[0];
}
__device__ __forceinline__ void scan1_padding(double (&v)[3], bool (&fl)[3]) {
    v[0] = v[1] = v[2] = 0;
    fl[0] = fl[1] = fl[2] = true;
}

template <class T>
__global__ __launch_bounds__(CT) void cox_batch_max_kernel(const T* __restrict__ base, const T* __restrict__ b0,
                                                           const T* __restrict__ off, BatchLayout L, double* __restrict__ scr) {
    __shared__ double red[NW];
    const int64_t n = L.n, l = blockIdx.y;
    const T* bl = base + size_t(l) * size_t(n);
    const T bb = b0[l];
    double m = -INFINITY;
    const int64_t first = int64_t(blockIdx.x) * TILE;
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int64_t i = first + int64_t(e) * CT + threadIdx.x;
        if (i < n) m = fmax(m, double(batch_eta(bl, bb, off, i)));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) m = fmax(m, __shfl_down(m, d, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = red[0];
        for (int w = 1; w < NW; ++w) r = fmax(r, red[w]);
        scr[L.pmax(l) + blockIdx.x] = r;
    }
}

// B2 for one pack.  FIRST: the rows and exp(eta - c) of this pack's stop / start positions are kept in rt / rs / xt / xs; the
// second pack takes them over wherever it names the same row, and gathers for itself where it does not.
template <class T, bool FIRST>
__device__ __forceinline__ void batch_scan1_up_pack(const CoxPack& pk, const T* __restrict__ bl, T bb, const T* __restrict__ off,
                                                    double c, int64_t b, int64_t (&rt)[CE], int64_t (&rs)[CE], double (&xt)[CE],
                                                    double (&xs)[CE], double* __restrict__ zto, double* __restrict__ zso,
                                                    double* __restrict__ agg, int64_t nt) {
    const int64_t n = pk.n;
    double v[CE][3];
    bool fl[CE][3];
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int64_t j = b * TILE + int64_t(threadIdx.x) * CE + e;
        if (j < n) {
            const int64_t q = n - 1 - j;
            const int64_t r1 = pk.to[q], r2 = pk.so[q];
            double x1, x2;
            if (FIRST) {
                rt[e] = r1; rs[e] = r2;
                xt[e] = x1 = exp(double(batch_eta(bl, bb, off, r1)) - c);
                xs[e] = x2 = exp(double(batch_eta(bl, bb, off, r2)) - c);
            } else {
                x1 = r1 == rt[e] ? xt[e] : exp(double(batch_eta(bl, bb, off, r1)) - c);
                x2 = r2 == rs[e] ? xs[e] : exp(double(batch_eta(bl, bb, off, r2)) - c);
            }
            const double zt = pk.w[r1] * x1;
            const double zs = pk.w[r2] * x2;
            zto[q] = zt;
            zso[q] = zs;
            scan1_channels(pk.flags[q], zt, zs, v[e], fl[e]);
        } else {
            scan1_padding(v[e], fl[e]);
        }
    }
    bool f[3], tf[3];
    double s[3], ts[3];
    thread_fold<3>(v, fl, f, s);
    block_seg_scan<3>(f, s, tf, ts);
    if (threadIdx.x < 3) {
        agg[b * 3 + threadIdx.x] = ts[threadIdx.x];
        agg[nt * 3 + b * 3 + threadIdx.x] = tf[threadIdx.x] ? 1.0 : 0.0;
    }
}

template <class T>
__global__ __launch_bounds__(CT) void cox_batch_scan1_up_kernel(CoxPack pa, CoxPack pb, const T* __restrict__ base,
                                                                const T* __restrict__ b0, const T* __restrict__ off,
                                                                BatchLayout L, double* __restrict__ scr) {
    const int64_t b = blockIdx.x, l = blockIdx.y;
    const T* bl = base + size_t(l) * size_t(L.n);
    const T bb = b0[l];
    const double c = fold_max(scr + L.pmax(l), L.nt);
    int64_t rt[CE], rs[CE];
    double xt[CE], xs[CE];
    batch_scan1_up_pack<T, true>(pa, bl, bb, off, c, b, rt, rs, xt, xs, scr + L.vec(l, 0, 0), scr + L.vec(l, 0, 1),
                                 scr + L.agg(l, 0), L.nt);
    batch_scan1_up_pack<T, false>(pb, bl, bb, off, c, b, rt, rs, xt, xs, scr + L.vec(l, 1, 0), scr + L.vec(l, 1, 1),
                                  scr + L.agg(l, 1), L.nt);
}

// B3 for one pack: z_to -> S_stop and z_so -> S_start in place, T_tie beside them
__device__ __forceinline__ void batch_scan1_down_pack(const CoxPack& pk, int64_t b, double* zto, double* zso,
                                                      double* __restrict__ ttie, const double* __restrict__ agg, int64_t nt) {
    const int64_t n = pk.n;
    double v[CE][3];
    bool fl[CE][3];
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int64_t j = b * TILE + int64_t(threadIdx.x) * CE + e;
        if (j < n) {
            const int64_t q = n - 1 - j;
            scan1_channels(pk.flags[q], zto[q], zso[q], v[e], fl[e]);
        } else {
            scan1_padding(v[e], fl[e]);
        }
    }
    bool f[3], tf[3], cf[3];
    double s[3], ts[3], cs[3];
    thread_fold<3>(v, fl, f, s);
    block_seg_scan<3>(f, s, tf, ts);
    tile_carry<3>(agg, nt, b, cf, cs);
#pragma unroll
    for (int k = 0; k < 3; ++k) seg_combine(cf[k], cs[k], f[k], s[k]); // incoming sum of the thread's first element
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int64_t j = b * TILE + int64_t(threadIdx.x) * CE + e;
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = fl[e][k] ? v[e][k] : s[k] + v[e][k];
        if (j < n) {
            const int64_t q = n - 1 - j;
            zto[q] = s[0];
            ttie[q] = s[1];
            zso[q] = s[2];
        }
    }
}

__global__ __launch_bounds__(CT) void cox_batch_scan1_down_kernel(CoxPack pa, CoxPack pb, BatchLayout L, double* scr) {
    const int64_t b = blockIdx.x, l = blockIdx.y;
    batch_scan1_down_pack(pa, b, scr + L.vec(l, 0, 0), scr + L.vec(l, 0, 1), scr + L.vec(l, 0, 2), scr + L.agg(l, 0), L.nt);
    batch_scan1_down_pack(pb, b, scr + L.vec(l, 1, 0), scr + L.vec(l, 1, 1), scr + L.vec(l, 1, 2), scr + L.agg(l, 1), L.nt);
}

// the log-risk part of one pack's loss over tile b (stop order): K4's risk totals and its sum, nothing else of K4
__device__ __forceinline__ double batch_log_risk(const CoxPack& pk, int64_t b, const double* __restrict__ s_stop,
                                                 const double* __restrict__ s_start, const double* __restrict__ t_tie,
                                                 double neg_max) {
    const int64_t n = pk.n;
    double lsum = 0;
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int64_t q = b * TILE + int64_t(threadIdx.x) * CE + e;
        if (q < n) {
            const uint8_t g = pk.flags[q];
            const double sc = pk.scale[q];
            const int64_t gs = pk.gstart[q], bp = pk.bpos[q];
            const double risk = s_stop[gs] - (bp >= 0 ? s_start[bp] : 0.0);
            const double rt = risk - sc * ((g & COX_IND) ? t_tie[gs] : 0.0);
            const double dw = pk.dw[q];
            if (dw != 0) lsum += dw * fmax(log(fmax(rt, 0.0)), neg_max);
        }
    }
    return block_sum(lsum);
}

template <class T>
__global__ __launch_bounds__(CT) void cox_batch_loss_parts_kernel(CoxPack pa, CoxPack pb, const T* __restrict__ base,
                                                                  const T* __restrict__ b0, const T* __restrict__ off,
                                                                  BatchLayout L, double* __restrict__ scr, double neg_max) {
    const int64_t n = L.n, b = blockIdx.x, l = blockIdx.y;
    const T* bl = base + size_t(l) * size_t(n);
    const T bb = b0[l];
    const double c = fold_max(scr + L.pmax(l), L.nt);
    const double ga = batch_log_risk(pa, b, scr + L.vec(l, 0, 0), scr + L.vec(l, 0, 1), scr + L.vec(l, 0, 2), neg_max);
    const double gb = batch_log_risk(pb, b, scr + L.vec(l, 1, 0), scr + L.vec(l, 1, 1), scr + L.vec(l, 1, 2), neg_max);
    double la = 0, lb = 0;
#pragma unroll
    for (int e = 0; e < CE; ++e) {
        const int64_t r = b * TILE + int64_t(e) * CT + threadIdx.x;
        if (r >= n) continue;
        const double er = double(batch_eta(bl, bb, off, r)) - c;
        la -= pa.wd[r] * er;
        lb -= pb.wd[r] * er;
    }
    la = block_sum(la);
    lb = block_sum(lb);
    if (threadIdx.x == 0) {
        scr[L.lossp(l, 0) + b] = ga;
        scr[L.lossp(l, 0) + L.nt + b] = la;
        scr[L.lossp(l, 1) + b] = gb;
        scr[L.lossp(l, 1) + L.nt + b] = lb;
    }
}

// grid (2, lc): pack blockIdx.x of lambda blockIdx.y
__global__ __launch_bounds__(CT) void cox_batch_loss_final_kernel(BatchLayout L, const double* __restrict__ scr,
                                                                  double* __restrict__ out) {
    const int64_t l = blockIdx.y;
    const int f = int(blockIdx.x);
    const double* part = scr + L.lossp(l, f);
    const int64_t m = 2 * L.nt;
    const int64_t chunk = (m + CT - 1) / CT;
    double s = 0;
    for (int64_t t = int64_t(threadIdx.x) * chunk; t < min(int64_t(threadIdx.x + 1) * chunk, m); ++t) s += part[t];
    s = block_sum(s);
    if (threadIdx.x == 0) out[size_t(l) * 2 + size_t(f)] = s;
}

} // namespace

size_t cox_scratch_doubles(int64_t n) { return Layout{n, n_tiles(n)}.total(); }
size_t cox_loss_slot(int64_t n) { return Layout{n, n_tiles(n)}.loss(); }

template <class T>
void cox_eval(const CoxPack& pk, const T* eta, T* grad, T* hess, bool want_loss, double* scratch, hipStream_t st) {
    const int64_t nt = n_tiles(pk.n);
    if (pk.n <= 0) return;
    const dim3 g(static_cast<unsigned>(nt)), blk(CT);
    const double neg_max = -double(std::numeric_limits<T>::max());
    hipLaunchKernelGGL(cox_max_kernel<T>, g, blk, 0, st, eta, pk.n, scratch + Layout{pk.n, nt}.pmax());
    hipLaunchKernelGGL((cox_scan1_kernel<T, false>), g, blk, 0, st, pk, eta, scratch);
    hipLaunchKernelGGL((cox_scan1_kernel<T, true>), g, blk, 0, st, pk, eta, scratch);
    hipLaunchKernelGGL((cox_scan2_kernel<T, false>), g, blk, 0, st, pk, scratch, neg_max);
    if (grad || hess) hipLaunchKernelGGL((cox_scan2_kernel<T, true>), g, blk, 0, st, pk, scratch, neg_max);
    hipLaunchKernelGGL(cox_combine_kernel<T>, g, blk, 0, st, pk, eta, grad, hess, scratch);
    if (want_loss) hipLaunchKernelGGL(cox_loss_final_kernel, dim3(1), blk, 0, st, scratch, pk.n);
    AHIP_CHECK(hipGetLastError());
}

template void cox_eval<float>(const CoxPack&, const float*, float*, float*, bool, double*, hipStream_t);
template void cox_eval<double>(const CoxPack&, const double*, double*, double*, bool, double*, hipStream_t);

size_t cox_loss_batch_scratch_doubles(int64_t n, int64_t lc) { return BatchLayout{n, n_tiles(n), lc}.total(); }

template <class T>
void cox_loss_batch(const CoxPack& pa, const CoxPack& pb, const T* base, const T* b0, const T* off, int64_t lc,
                    double* scratch, double* out, hipStream_t st) {
    if (pa.n != pb.n) throw make_core_error("cox_loss_batch: the two families have different numbers of rows.");
    if (lc > 65535) throw make_core_error("cox_loss_batch: at most 65535 etas per call.");
    if (pa.n <= 0 || lc <= 0) return;
    const BatchLayout L{pa.n, n_tiles(pa.n), lc};
    const dim3 g(static_cast<unsigned>(L.nt), static_cast<unsigned>(lc)), blk(CT);
    const double neg_max = -double(std::numeric_limits<T>::max());
    hipLaunchKernelGGL(cox_batch_max_kernel<T>, g, blk, 0, st, base, b0, off, L, scratch);
    hipLaunchKernelGGL(cox_batch_scan1_up_kernel<T>, g, blk, 0, st, pa, pb, base, b0, off, L, scratch);
    hipLaunchKernelGGL(cox_batch_scan1_down_kernel, g, blk, 0, st, pa, pb, L, scratch);
    hipLaunchKernelGGL(cox_batch_loss_parts_kernel<T>, g, blk, 0, st, pa, pb, base, b0, off, L, scratch, neg_max);
    hipLaunchKernelGGL(cox_batch_loss_final_kernel, dim3(2, static_cast<unsigned>(lc)), blk, 0, st, L, scratch, out);
    AHIP_CHECK(hipGetLastError());
}

template void cox_loss_batch<float>(const CoxPack&, const CoxPack&, const float*, const float*, const float*, int64_t, double*,
                                    double*, hipStream_t);
template void cox_loss_batch<double>(const CoxPack&, const CoxPack&, const double*, const double*, const double*, int64_t,
                                     double*, double*, hipStream_t);

// ---------------------------------------------------------------------------------------------------------------------
// The pack, built on the host (glm_cox.ipp:214-354, 519-597 restated on stratum-segmented global arrays)
template <class T>
static adelie_hip_glm_cox* cox_build(int device, int64_t n, const T* start, const T* stop, const T* status,
                                     const int64_t* strata, const T* weights, int tie_method) {
    const size_t N = size_t(n);
    std::vector<int64_t> st(N, 0);
    if (strata) {
        for (int64_t i = 0; i < n; ++i) {
            if (strata[i] < 0) throw make_core_error("strata must take values in {0, ..., M-1}.");
            st[size_t(i)] = strata[i];
        }
    }
    std::vector<int64_t> to(N), so(N);
    std::iota(to.begin(), to.end(), int64_t(0));
    std::iota(so.begin(), so.end(), int64_t(0));
    std::stable_sort(to.begin(), to.end(), [&](int64_t i, int64_t j) {
        return st[size_t(i)] < st[size_t(j)] || (st[size_t(i)] == st[size_t(j)] && stop[i] < stop[j]);
    });
    std::stable_sort(so.begin(), so.end(), [&](int64_t i, int64_t j) {
        return st[size_t(i)] < st[size_t(j)] || (st[size_t(i)] == st[size_t(j)] && start[i] < start[j]);
    });
    std::vector<double> stop_to(N), start_so(N);
    for (int64_t q = 0; q < n; ++q) {
        stop_to[size_t(q)] = double(stop[to[size_t(q)]]);
        start_so[size_t(q)] = double(start[so[size_t(q)]]);
    }
    std::vector<uint8_t> flags(N, 0);
    std::vector<int64_t> gstart(N), gend(N), bpos(N), ub_m1(N);
    std::vector<double> ind_to(N), w_to(N), d_to(N);
    for (int64_t q = 0; q < n; ++q) {
        const int64_t r = to[size_t(q)];
        w_to[size_t(q)] = double(weights[r]);
        d_to[size_t(q)] = double(status[r]);
        ind_to[size_t(q)] = d_to[size_t(q)] * double(weights[r] != T(0));
    }
    for (int64_t lo = 0; lo < n;) { // one stratum [lo, hi)
        const int64_t s = st[size_t(to[size_t(lo)])];
        int64_t hi = lo;
        while (hi < n && st[size_t(to[size_t(hi)])] == s) ++hi;
        flags[size_t(lo)] |= COX_STRATUM_FIRST;
        flags[size_t(hi - 1)] |= COX_STRATUM_LAST;
        const double* ss = start_so.data();
        const double* tt = stop_to.data();
        for (int64_t q = lo; q < hi; ++q) {
            const int64_t b = std::lower_bound(ss + lo, ss + hi, tt[q]) - ss;
            bpos[size_t(q)] = b < hi ? b : -1;
            const int64_t u = std::upper_bound(tt + lo, tt + hi, ss[q]) - tt;
            ub_m1[size_t(q)] = u > lo ? u - 1 : -1;
        }
        for (int64_t g0 = lo; g0 < hi;) { // tie groups
            int64_t g1 = g0;
            while (g1 < hi && stop_to[size_t(g1)] == stop_to[size_t(g0)]) ++g1;
            flags[size_t(g0)] |= COX_TIE_FIRST;
            flags[size_t(g1 - 1)] |= COX_TIE_LAST;
            for (int64_t q = g0; q < g1; ++q) { gstart[size_t(q)] = g0; gend[size_t(q)] = g1; }
            g0 = g1;
        }
        lo = hi;
    }
    // tie sizes, averaged weights and scales over the events with non-zero weight (glm_cox.ipp:151-264, 302-354)
    std::vector<double> scale(N, 0.0), dw(N, 0.0);
    for (int64_t g0 = 0; g0 < n; g0 = gend[size_t(g0)]) {
        const int64_t g1 = gend[size_t(g0)];
        double size = 0, wsum = 0;
        for (int64_t q = g0; q < g1; ++q) {
            if (ind_to[size_t(q)] != 0) {
                if (tie_method == ADELIE_HIP_TIE_EFRON) scale[size_t(q)] = size * ind_to[size_t(q)];
                size += ind_to[size_t(q)];
                wsum += w_to[size_t(q)] * ind_to[size_t(q)];
            }
        }
        for (int64_t q = g0; q < g1; ++q) {
            if (size > 0) scale[size_t(q)] /= size;
            const double wbar = (ind_to[size_t(q)] != 0 && size > 0) ? wsum / size : 0.0;
            dw[size_t(q)] = d_to[size_t(q)] * wbar;
            if (ind_to[size_t(q)] != 0) flags[size_t(q)] |= COX_IND;
        }
    }
    std::vector<int64_t> inv_to(N), inv_so(N), row_a(N), row_b(N);
    for (int64_t q = 0; q < n; ++q) { inv_to[size_t(to[size_t(q)])] = q; inv_so[size_t(so[size_t(q)])] = q; }
    std::vector<double> w(N), wd(N), ind(N);
    for (int64_t r = 0; r < n; ++r) {
        row_a[size_t(r)] = gend[size_t(inv_to[size_t(r)])] - 1;
        row_b[size_t(r)] = ub_m1[size_t(inv_so[size_t(r)])];
        w[size_t(r)] = double(weights[r]);
        wd[size_t(r)] = double(weights[r]) * double(status[r]);
        ind[size_t(r)] = double(status[r]) * double(weights[r] != T(0));
    }
    // one device block: 6 int64 arrays, 5 double arrays, the flags
    const size_t bytes = N * (6 * sizeof(int64_t) + 5 * sizeof(double)) + N + 64;
    AHIP_CHECK(hipSetDevice(device));
    auto* h = new adelie_hip_glm_cox();
    h->device = device;
    h->dtype = std::is_same<T, double>::value ? ADELIE_HIP_F64 : ADELIE_HIP_F32;
    if (hipMalloc(&h->block, bytes) != hipSuccess) {
        delete h;
        throw make_core_error("glm_cox: device allocation failed.");
    }
    std::vector<char> host(bytes, 0);
    size_t off = 0;
    auto put = [&](const void* src, size_t sz) {
        std::memcpy(host.data() + off, src, sz);
        const size_t at = off;
        off += sz;
        return static_cast<char*>(h->block) + at;
    };
    CoxPack& pk = h->pack;
    pk.n = n;
    pk.to = reinterpret_cast<const int64_t*>(put(to.data(), N * 8));
    pk.so = reinterpret_cast<const int64_t*>(put(so.data(), N * 8));
    pk.gstart = reinterpret_cast<const int64_t*>(put(gstart.data(), N * 8));
    pk.bpos = reinterpret_cast<const int64_t*>(put(bpos.data(), N * 8));
    pk.row_a = reinterpret_cast<const int64_t*>(put(row_a.data(), N * 8));
    pk.row_b = reinterpret_cast<const int64_t*>(put(row_b.data(), N * 8));
    pk.scale = reinterpret_cast<const double*>(put(scale.data(), N * 8));
    pk.dw = reinterpret_cast<const double*>(put(dw.data(), N * 8));
    pk.w = reinterpret_cast<const double*>(put(w.data(), N * 8));
    pk.wd = reinterpret_cast<const double*>(put(wd.data(), N * 8));
    pk.ind = reinterpret_cast<const double*>(put(ind.data(), N * 8));
    pk.flags = reinterpret_cast<const uint8_t*>(put(flags.data(), N));
    const hipError_t e = hipMemcpy(h->block, host.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(h->block);
        delete h;
        throw make_core_error(std::string("glm_cox: upload failed: ") + hipGetErrorString(e));
    }
    return h;
}

adelie_hip_glm_cox* cox_create(int device, int dtype, int64_t n, const void* start, const void* stop, const void* status,
                               const int64_t* strata, const void* weights, int tie_method) {
    if (n < 1) throw make_core_error("glm_cox: n must be >= 1.");
    if (!start || !stop || !status || !weights) throw make_core_error("null argument.");
    if (tie_method != ADELIE_HIP_TIE_BRESLOW && tie_method != ADELIE_HIP_TIE_EFRON)
        throw make_core_error("Invalid tie method.");
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
        throw make_core_error("no HIP device is visible: adelie_hip has no CPU fallback.");
    if (device < 0 || device >= cnt) throw make_core_error("device ordinal out of range.");
    if (dtype == ADELIE_HIP_F64)
        return cox_build<double>(device, n, static_cast<const double*>(start), static_cast<const double*>(stop),
                                 static_cast<const double*>(status), strata, static_cast<const double*>(weights), tie_method);
    if (dtype == ADELIE_HIP_F32)
        return cox_build<float>(device, n, static_cast<const float*>(start), static_cast<const float*>(stop),
                                static_cast<const float*>(status), strata, static_cast<const float*>(weights), tie_method);
    throw make_core_error("dtype must be ADELIE_HIP_F32 or ADELIE_HIP_F64.");
}

void cox_destroy(adelie_hip_glm_cox* h) {
    if (!h) return;
    if (h->block) {
        (void)hipSetDevice(h->device);
        (void)hipFree(h->block);
    }
    delete h;
}

// adelie_hip_glm_cox_eval: host arrays in and out, own stream and scratch
template <class T>
static void cox_eval_host_t(const adelie_hip_glm_cox* h, const void* eta, void* grad, void* hess, double* loss) {
    const int64_t n = h->pack.n;
    AHIP_CHECK(hipSetDevice(h->device));
    DevBuf<double> scr;
    DevBuf<T> d_eta, d_g, d_h;
    hipStream_t st;
    AHIP_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    // (destroyed before the buffers: they are parked only once nothing on the stream can still use them)
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } } sg{st};
    scr.reserve(cox_scratch_doubles(n));
    d_eta.reserve(size_t(n));
    if (grad) d_g.reserve(size_t(n));
    if (hess) d_h.reserve(size_t(n));
    AHIP_CHECK(hipMemcpyAsync(d_eta.p, eta, size_t(n) * sizeof(T), hipMemcpyHostToDevice, st));
    cox_eval<T>(h->pack, d_eta.p, grad ? d_g.p : nullptr, hess ? d_h.p : nullptr, loss != nullptr, scr.p, st);
    if (grad) AHIP_CHECK(hipMemcpyAsync(grad, d_g.p, size_t(n) * sizeof(T), hipMemcpyDeviceToHost, st));
    if (hess) AHIP_CHECK(hipMemcpyAsync(hess, d_h.p, size_t(n) * sizeof(T), hipMemcpyDeviceToHost, st));
    if (loss) AHIP_CHECK(hipMemcpyAsync(loss, scr.p + cox_loss_slot(n), sizeof(double), hipMemcpyDeviceToHost, st));
    AHIP_CHECK(hipStreamSynchronize(st));
}

void cox_eval_host(const adelie_hip_glm_cox* h, const void* eta, void* grad, void* hess, double* loss) {
    if (!h || !eta) throw make_core_error("null argument.");
    if (h->dtype == ADELIE_HIP_F64) cox_eval_host_t<double>(h, eta, grad, hess, loss);
    else cox_eval_host_t<float>(h, eta, grad, hess, loss);
}

} // namespace ahip
