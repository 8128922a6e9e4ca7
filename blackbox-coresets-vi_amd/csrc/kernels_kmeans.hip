// kernels_kmeans.hip -- psvi_kmeans: k-means++ seeding on the library's
// Philox stream and Lloyd iterations over rows x [N][D] (fp32, widened exactly)
// with fp64 centres; the rules are stated in include/psvi_hip.h.
//
// Launches, all ordinary (no workgroup waits for another inside a launch):
//   seeding   km_seed_first, then per further centre km_seed_dist (every
//             workgroup: m_i = min(m_i, d(i, newest centre)), the totals of its
//             runs of 64 rows) and km_seed_pick (one workgroup: the run prefix
//             in run order, t = U C_{N-1}, the row, the new centre)
//   iteration km_assign (labels, per-workgroup inertia / counts / "a label
//             changed", and -- one-pass sums -- the per-workgroup cluster sums
//             of its own rows), km_sums (the second-pass sums, when the
//             workspace holds fewer partials than assignment workgroups), and
//             km_combine (the convergence test, made by every workgroup from
//             the same numbers in the same order, then the new centres)
//   km_finish labels -1 when the status is not 0
// `done` is a pair of device words: launch t reads done[t & 1], km_combine's
// first workgroup writes done[(t + 1) & 1], so no workgroup reads a word that
// its own launch writes.  Once it is set every later launch returns at once;
// the host reads it once per kKmChunk iterations.
// Nothing that decides a label, a centre, the inertia or a seed goes through
// an atomic: every sum has one owner and a fixed order.
#include <limits.h>

#include "lds_layout.hpp"

namespace psvi {

namespace {

constexpr int kKg = kKmThreads / kKmRows;  // centre groups of a row: one wave each

struct KmState {
    int done[2];
};

// the workspace of a call
struct KmWs {
    KmState* state;
    double *m, *runT, *runB;
    int *runLast, *runBad, *changed, *bad;
    double* inertia;
    int* cnt;       // [G][K]
    double* shift[2];  // [cy][K]: update t writes shift[t & 1], test t + 1 reads it
    double* part;   // [P][K][D]: the rest of the workspace
};

// s: the grids of kmeans_shape; fixed: the bytes before the partials (base
// nullptr: sizes only)
KmWs km_carve(void* base, const KmeansShape& s, int64_t N, int K, size_t* fixed = nullptr) {
    WsCarve c(base);
    KmWs w;
    w.state = c.take<KmState>(1);                  // the state words
    w.m = c.take<double>((size_t)N);               // the seeding's distances
    w.runT = c.take<double>((size_t)s.nruns);      // run totals
    w.runB = c.take<double>((size_t)s.nruns);      // run prefix
    w.runLast = c.take<int>((size_t)s.nruns);      // last positive row
    w.runBad = c.take<int>((size_t)s.nruns);       // non-finite flag
    w.changed = c.take<int>((size_t)s.G);
    w.bad = c.take<int>((size_t)s.G);
    w.inertia = c.take<double>((size_t)s.G);
    w.cnt = c.take<int>((size_t)s.G * K);
    for (double*& sh : w.shift) sh = c.take<double>((size_t)K * s.cy);  // of even / odd updates
    w.part = c.take<double>(0);
    if (fixed) *fixed = c.bytes();
    return w;
}

struct KmArgs {
    const float* x;
    int N, D, K;
    uint64_t seed, offset;
    int max_iter;
    double tol;
    double* centres;
    int32_t *labels, *counts, *seeds;
    double* inertia_out;
    int32_t *n_iter, *status;
    KmWs w;
    int DT, XS, tpb, G, nruns, cy;
    int P;       // partials of the cluster sums
    int rpc;     // rows per partial of the second-pass sums (0: one-pass, partial = workgroup)
};

__device__ __forceinline__ bool km_finite(double d) { return d < INFINITY && d > -INFINITY; }

// ------------------------------------------------------------------ seeding
// centres <- centres_in, seeds <- -1
__global__ __launch_bounds__(kKmThreads) void km_copy_kernel(KmArgs a, const double* src) {
    const int64_t n = (int64_t)a.K * a.D;
    for (int64_t e = (int64_t)blockIdx.x * kKmThreads + threadIdx.x; e < n;
         e += (int64_t)gridDim.x * kKmThreads)
        a.centres[e] = src[e];
    if (blockIdx.x == 0 && a.seeds)
        for (int k = threadIdx.x; k < a.K; k += kKmThreads) a.seeds[k] = -1;
}

// centre j <- row i, widened
__device__ __forceinline__ void km_take_row(const KmArgs& a, int j, int i) {
    const float* __restrict__ src = a.x + (int64_t)i * a.D;
    double* dst = a.centres + (int64_t)j * a.D;
    for (int f = threadIdx.x; f < a.D; f += kKmThreads) dst[f] = (double)src[f];
}

// centre 0: row floor(U_0 N), clamped
__global__ __launch_bounds__(kKmThreads) void km_seed_first_kernel(KmArgs a) {
    uint32_t c[4];
    draw_words(a.seed, a.offset, 0, c);
    const int i = min((int)(draw_uniform(c[0]) * (double)a.N), a.N - 1);
    if (threadIdx.x == 0) {
        a.status[0] = 0;
        if (a.seeds) {
            a.seeds[0] = i;
            for (int k = 1; k < a.K; ++k) a.seeds[k] = -1;
        }
    }
    km_take_row(a, 0, i);
}

// m_i = min(m_i, d(i, centre j - 1)) (j == 1: = d), and per run of 64 rows its
// total in index order, its last row with m_i > 0 and whether a distance is
// not finite
__global__ __launch_bounds__(kKmThreads) void km_seed_dist_kernel(KmArgs a, int j) {
    __shared__ double sCen[kKmMaxD];
    __shared__ double sM[kKmRows];
    if (a.status[0] != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wid = wave_id();
    const double* cen = a.centres + (int64_t)(j - 1) * a.D;
    for (int f = tid; f < a.D; f += kKmThreads) sCen[f] = cen[f];
    __syncthreads();
    for (int run = blockIdx.x; run < a.nruns; run += gridDim.x) {
        for (int rr = wid; rr < kKmRows; rr += kKg) {
            const int row = run * kKmRows + rr;
            if (row >= a.N) {
                if (lane == 0) sM[rr] = -1.0;  // no such row
                continue;
            }
            const float* __restrict__ xr = a.x + (int64_t)row * a.D;
            double d = 0.0;
            for (int f = lane; f < a.D; f += kWave) {
                const double diff = (double)xr[f] - sCen[f];
                d = fma(diff, diff, d);
            }
            d = wave_sum(d);
            if (lane == 0) {
                double mi = d;
                if (j > 1 && km_finite(d)) {
                    const double mo = a.w.m[row];
                    mi = d < mo ? d : mo;
                }
                a.w.m[row] = mi;
                sM[rr] = mi;
            }
        }
        __syncthreads();
        if (tid == 0) {
            double tot = 0.0;
            int last = -1, bad = 0;
            for (int rr = 0; rr < kKmRows; ++rr) {
                const double mi = sM[rr];
                if (mi == -1.0) break;
                bad |= !km_finite(mi);
                tot += mi;
                if (mi > 0.0) last = run * kKmRows + rr;
            }
            a.w.runT[run] = tot;
            a.w.runLast[run] = last;
            a.w.runBad[run] = bad;
        }
        __syncthreads();
    }
}

// centre j: C_i = (the totals of the runs before i's, added in run order) +
// (m summed in index order within the run); t = U_{4j} C_{N-1}; the smallest i
// with C_i > t, clamped to the last i with m_i > 0
__global__ __launch_bounds__(kKmThreads) void km_seed_pick_kernel(KmArgs a, int j) {
    __shared__ double red[kKmThreads];
    __shared__ int sPick;
    if (a.status[0] != 0) return;
    const int tid = threadIdx.x;
    if (tid == 0) {
        double acc = 0.0;
        for (int r = 0; r < a.nruns; ++r) {
            acc += a.w.runT[r];
            a.w.runB[r] = acc;
        }
    }
    int bad = 0;
    double last = -1.0;
    for (int r = tid; r < a.nruns; r += kKmThreads) {
        bad |= a.w.runBad[r];
        last = fmax(last, (double)a.w.runLast[r]);
    }
    bad = __syncthreads_or(bad);  // also orders thread 0's runB before its readers
    const int lastpos = (int)tree_max<kKmThreads>(last, red);
    if (bad || lastpos < 0) {
        if (tid == 0) {
            a.status[0] = bad ? 1 : 2;
            a.w.state->done[0] = a.w.state->done[1] = 1;
        }
        return;
    }
    uint32_t c[4];
    draw_words(a.seed, a.offset, j, c);
    const double t = draw_uniform(c[0]) * a.w.runB[a.nruns - 1];
    double first = -(double)(a.nruns - 1);  // minus the first run whose closing prefix exceeds t
    for (int r = a.nruns - 1 - tid; r >= 0; r -= kKmThreads)
        if (a.w.runB[r] > t) first = fmax(first, -(double)r);
    const int run = (int)(-tree_max<kKmThreads>(first, red));
    if (tid == 0) {
        const double before = run > 0 ? a.w.runB[run - 1] : 0.0;
        const int lo = run * kKmRows, hi = min(lo + kKmRows, a.N);
        double within = 0.0;
        int i = hi - 1;
        for (int q = lo; q < hi; ++q) {
            within += a.w.m[q];
            if (before + within > t) {
                i = q;
                break;
            }
        }
        i = min(i, lastpos);
        sPick = i;
        if (a.seeds) a.seeds[j] = i;
    }
    __syncthreads();
    km_take_row(a, j, sPick);
}

// ----------------------------------------------------------------- iteration
// out[k][f0 + c] <- the sum of the rows [row_lo, row_hi) with label k, columns
// [f0, f0 + dt), in row order: thread c owns column c of every cluster
__device__ __forceinline__ void km_accumulate(const KmArgs& a, int row_lo, int row_hi, int f0,
                                              int dt, double* sAcc, int* sLab, double* out) {
    const int tid = threadIdx.x, DT = a.DT;
    for (int e = tid; e < a.K * DT; e += kKmThreads) sAcc[e] = 0.0;
    for (int base = row_lo; base < row_hi; base += kKmRows) {
        __syncthreads();
        if (tid < kKmRows) sLab[tid] = base + tid < row_hi ? a.labels[base + tid] : -1;
        __syncthreads();
        const int nr = min(kKmRows, row_hi - base);
        for (int c = tid; c < dt; c += kKmThreads) {
            const float* __restrict__ xp = a.x + (int64_t)base * a.D + f0 + c;
#pragma unroll 4
            for (int r = 0; r < nr; ++r) sAcc[sLab[r] * DT + c] += (double)xp[(int64_t)r * a.D];
        }
    }
    __syncthreads();
    for (int k = wave_id(); k < a.K; k += kKg)
        for (int c = tid & 63; c < dt; c += kWave) out[(int64_t)k * a.D + f0 + c] = sAcc[k * DT + c];
    __syncthreads();
}

// Labels of the workgroup's row tiles against the centres: per tile of 64 rows
// and per tile of DT columns the centres (fp64) and the rows (fp32) are staged
// in LDS; thread (r, g) holds d(r, k) for k = g, g + 4, ...  Then, one-pass
// sums only, the cluster sums of the workgroup's own rows (read again while
// they are still in cache).
template <int KPT>
__global__ __launch_bounds__(kKmThreads) void km_assign_kernel(KmArgs a, int t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char km_sm[];
    __shared__ double sBd[kKg][kKmRows];
    __shared__ int sBk[kKg][kKmRows];
    __shared__ int sLab[kKmRows];
    __shared__ int sCnt[kKmMaxK];
    if (a.w.state->done[t & 1]) return;
    const KmLds sh = km_lds(km_sm, a.K, a.DT, a.XS, true);
    double* sC = sh.sC;
    float* sX = sh.sX;
    const int tid = threadIdx.x, lane = tid & 63, g = wave_id();
    const int K = a.K, D = a.D, DT = a.DT, XS = a.XS;
    const int nk = g < K ? (K - g + kKg - 1) / kKg : 0;
    const int tile_lo = blockIdx.x * a.tpb, tile_hi = min(tile_lo + a.tpb, (a.N + kKmRows - 1) / kKmRows);
    for (int k = tid; k < K; k += kKmThreads) sCnt[k] = 0;
    double inertia = 0.0;  // lane 0 of wave 0: the tiles' sums in tile order
    int changed = 0, bad = 0;
    for (int tile = tile_lo; tile < tile_hi; ++tile) {
        const int row0 = tile * kKmRows;
        double acc[KPT];
#pragma unroll
        for (int q = 0; q < KPT; ++q) acc[q] = 0.0;
        for (int f0 = 0; f0 < D; f0 += DT) {
            const int dt = min(DT, D - f0);
            __syncthreads();
            for (int k = g; k < K; k += kKg)
                for (int c = lane; c < dt; c += kWave) sC[k * DT + c] = a.centres[(int64_t)k * D + f0 + c];
            for (int r = g; r < kKmRows; r += kKg) {
                const int row = row0 + r;
                const float* __restrict__ xr = a.x + (int64_t)row * D + f0;
                for (int c = lane; c < dt; c += kWave) sX[r * XS + c] = row < a.N ? xr[c] : 0.f;
            }
            __syncthreads();
            const float* xrow = sX + lane * XS;
            for (int c = 0; c < dt; ++c) {
                const double xv = (double)xrow[c];
#pragma unroll
                for (int q = 0; q < KPT; ++q)
                    if (q < nk) {
                        const double diff = xv - sC[(g + kKg * q) * DT + c];
                        acc[q] = fma(diff, diff, acc[q]);
                    }
            }
        }
        // the lowest k among equal distances: ascending k within the thread,
        // (d, k) pairs across the four groups
        double bd = INFINITY;
        int bk = INT_MAX, nf = 0;
#pragma unroll
        for (int q = 0; q < KPT; ++q)
            if (q < nk) {
                nf |= !km_finite(acc[q]);
                if (acc[q] < bd || bk == INT_MAX) {
                    bd = acc[q];
                    bk = g + kKg * q;
                }
            }
        sBd[g][lane] = bd;
        sBk[g][lane] = bk;
        bad |= nf && row0 + lane < a.N;
        __syncthreads();
        if (g == 0) {
            const int row = row0 + lane;
#pragma unroll
            for (int q = 1; q < kKg; ++q) {
                const double d = sBd[q][lane];
                const int k = sBk[q][lane];
                if (k != INT_MAX && (d < bd || (d == bd && k < bk))) {
                    bd = d;
                    bk = k;
                }
            }
            const bool live = row < a.N;
            if (live) {
                changed |= a.labels[row] != bk;
                a.labels[row] = bk;
            }
            sLab[lane] = live ? bk : -1;
            const double s = wave_sum(live ? bd : 0.0);
            inertia += s;
        }
        __syncthreads();
        if (tid < K) {
            int n = 0;
            for (int r = 0; r < kKmRows; ++r) n += sLab[r] == tid;
            sCnt[tid] += n;
        }
    }
    bad = __syncthreads_or(bad);
    changed = __syncthreads_or(changed);
    if (tid == 0) {
        a.w.inertia[blockIdx.x] = inertia;
        a.w.changed[blockIdx.x] = changed;
        a.w.bad[blockIdx.x] = bad;
    }
    for (int k = tid; k < K; k += kKmThreads) a.w.cnt[(int64_t)blockIdx.x * K + k] = sCnt[k];
    if (a.rpc == 0) {
        // __syncthreads above: the labels this workgroup wrote are visible to it
        double* out = a.w.part + (int64_t)blockIdx.x * K * D;
        for (int f0 = 0; f0 < D; f0 += DT)
            km_accumulate(a, tile_lo * kKmRows, min(tile_hi * kKmRows, a.N), f0, min(DT, D - f0), sC,
                          sLab, out);
    }
}

// the second-pass sums: workgroup (p, ct) owns the rows of chunk p and the
// columns of tile ct
__global__ __launch_bounds__(kKmThreads) void km_sums_kernel(KmArgs a, int t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char km_sm[];
    __shared__ int sLab[kKmRows];
    if (a.w.state->done[t & 1]) return;
    const int p = blockIdx.x, f0 = blockIdx.y * a.DT;
    const int row_lo = (int)min((int64_t)p * a.rpc, (int64_t)a.N);
    const int row_hi = (int)min((int64_t)row_lo + a.rpc, (int64_t)a.N);
    km_accumulate(a, row_lo, row_hi, f0, min(a.DT, a.D - f0), km_lds(km_sm, a.K, a.DT, a.XS, false).sC,
                  sLab, a.w.part + (int64_t)p * a.K * a.D);
}

// Workgroup (k, cb): columns [256 cb, 256 cb + 256) of centre k.  Every
// workgroup makes the same test from the same partials in the same order: a
// non-finite distance (status 1), the final assignment (t == max_iter, or the
// last update's summed squared shift <= tol), no label changed (t > 0).  On a
// stop the first workgroup of a row writes counts / inertia / n_iter; else
// centre k <- the partial sums in partial order / count (count 0: kept).
__global__ __launch_bounds__(kKmThreads) void km_combine_kernel(KmArgs a, int t) {
    __shared__ double red[kKmThreads];
    const int tid = threadIdx.x, k = blockIdx.x, cb = blockIdx.y, K = a.K;
    const bool first = k == 0 && cb == 0 && tid == 0;
    if (a.w.state->done[t & 1]) {
        if (first) a.w.state->done[(t + 1) & 1] = 1;
        return;
    }
    int ch = 0, bd = 0;
    double cn = 0.0;  // a count: exact in fp64
    for (int b = tid; b < a.G; b += kKmThreads) {
        ch |= a.w.changed[b];
        bd |= a.w.bad[b];
        cn += (double)a.w.cnt[(int64_t)b * K + k];
    }
    ch = __syncthreads_or(ch);
    bd = __syncthreads_or(bd);
    const double count = tree_sum<kKmThreads>(cn, red);
    double shift = 0.0;
    if (t > 0) {
        double s = 0.0;
        const double* prev = a.w.shift[(t - 1) & 1];
        for (int e = tid; e < K * a.cy; e += kKmThreads) s += prev[e];
        shift = tree_sum<kKmThreads>(s, red);
    }
    const bool final = t == a.max_iter || (t > 0 && shift <= a.tol);
    const bool same = t > 0 && !ch;
    if (bd) {
        if (first) {
            a.status[0] = 1;
            a.w.state->done[(t + 1) & 1] = 1;
        }
        return;
    }
    if (final || same) {
        if (cb == 0 && tid == 0) a.counts[k] = (int)count;
        if (k == 0 && cb == 0) {
            double s = 0.0;
            for (int b = tid; b < a.G; b += kKmThreads) s += a.w.inertia[b];
            s = tree_sum<kKmThreads>(s, red);
            if (tid == 0) {
                a.inertia_out[0] = s;
                a.n_iter[0] = final ? t : t + 1;
                a.w.state->done[(t + 1) & 1] = 1;
            }
        }
        return;
    }
    const int f = cb * kKmThreads + tid;
    double sq = 0.0;
    if (f < a.D && count > 0.0) {
        const double* part = a.w.part + (int64_t)k * a.D + f;
        double s = 0.0;
        for (int p = 0; p < a.P; ++p) s += part[(int64_t)p * K * a.D];
        const double cnew = s / count, diff = cnew - a.centres[(int64_t)k * a.D + f];
        a.centres[(int64_t)k * a.D + f] = cnew;
        sq = diff * diff;
    }
    sq = tree_sum<kKmThreads>(sq, red);
    if (tid == 0) a.w.shift[t & 1][cb * K + k] = sq;
    if (first) a.w.state->done[(t + 1) & 1] = 0;
}

// a status other than 0: labels -1, counts 0, inertia 0, n_iter 0
__global__ __launch_bounds__(kKmThreads) void km_finish_kernel(KmArgs a) {
    if (a.status[0] == 0) return;
    for (int64_t i = (int64_t)blockIdx.x * kKmThreads + threadIdx.x; i < a.N;
         i += (int64_t)gridDim.x * kKmThreads)
        a.labels[i] = -1;
    if (blockIdx.x == 0) {
        for (int k = threadIdx.x; k < a.K; k += kKmThreads) a.counts[k] = 0;
        if (threadIdx.x == 0) {
            a.inertia_out[0] = 0.0;
            a.n_iter[0] = 0;
        }
    }
}

typedef void (*km_assign_fn)(KmArgs, int);
km_assign_fn km_assign_for(int K) {
    const int kpt = (K + kKg - 1) / kKg;
    if (kpt <= 1) return km_assign_kernel<1>;
    if (kpt <= 2) return km_assign_kernel<2>;
    if (kpt <= 4) return km_assign_kernel<4>;
    if (kpt <= 8) return km_assign_kernel<8>;
    if (kpt <= 16) return km_assign_kernel<16>;
    return km_assign_kernel<32>;
}

}  // namespace

KmeansShape kmeans_shape(int64_t N, int D, int K) {
    KmeansShape s;
    s.DT = km_tile_cols(D, K);
    s.XS = s.DT | 1;
    s.tiles = (int)((N + kKmRows - 1) / kKmRows);
    s.tpb = (s.tiles + kKmMaxGrid - 1) / kKmMaxGrid;
    s.G = (s.tiles + s.tpb - 1) / s.tpb;
    s.nruns = s.tiles;
    s.cy = (D + kKmThreads - 1) / kKmThreads;
    s.part = align256(sizeof(double) * (size_t)K * D);
    km_carve(nullptr, s, N, K, &s.fixed);
    s.min_bytes = s.fixed + s.part;
    s.full_bytes = s.fixed + (size_t)s.G * s.part;
    return s;
}

hipError_t launch_kmeans(const Kmeans& r, hipStream_t st) {
    const KmeansShape s = kmeans_shape(r.N, r.D, r.K);
    if (!r.x || !r.centres || !r.labels || !r.counts || !r.inertia || !r.n_iter || !r.status ||
        !r.ws || r.ws_bytes < s.min_bytes || r.N < 1 || r.K < 1 || r.K > r.N || r.K > kKmMaxK ||
        r.D < 1 || r.D > kKmMaxD || r.N > kKmMaxN || r.max_iter < 0)
        return hipErrorInvalidValue;
    KmArgs a;
    a.x = r.x; a.N = r.N; a.D = r.D; a.K = r.K;
    a.seed = r.seed; a.offset = r.offset; a.max_iter = r.max_iter; a.tol = r.tol;
    a.centres = r.centres; a.labels = r.labels; a.counts = r.counts; a.seeds = r.seeds;
    a.inertia_out = r.inertia; a.n_iter = r.n_iter; a.status = r.status;
    a.w = km_carve(r.ws, s, r.N, r.K);
    a.DT = s.DT; a.XS = s.XS; a.tpb = s.tpb; a.G = s.G; a.nruns = s.nruns; a.cy = s.cy;
    const size_t fit = (r.ws_bytes - s.fixed) / s.part;
    if (fit >= (size_t)s.G) {
        a.P = s.G;
        a.rpc = 0;
    } else {
        // chunks of whole tiles, as many as the workspace holds
        const int want = (int)std::min<size_t>(fit, kKmMaxParts);
        const int tiles_per = (s.tiles + want - 1) / want;
        a.rpc = tiles_per * kKmRows;
        a.P = (s.tiles + tiles_per - 1) / tiles_per;
    }
    const km_assign_fn assign = km_assign_for(r.K);
    const size_t lds_assign = km_lds(nullptr, r.K, s.DT, s.XS, true).bytes;
    const size_t lds_sums = km_lds(nullptr, r.K, s.DT, s.XS, false).bytes;
    if (hipError_t e = allow_dynamic_lds((const void*)assign, kKmLds); e != hipSuccess) return e;
    if (hipError_t e = allow_dynamic_lds((const void*)km_sums_kernel, kKmLds); e != hipSuccess)
        return e;
    if (hipError_t e = hipMemsetAsync(a.w.state, 0, sizeof(KmState), st); e != hipSuccess) return e;
    const dim3 T(kKmThreads);
    if (r.centres_in) {
        if (hipError_t e = hipMemsetAsync(r.status, 0, sizeof(int32_t), st); e != hipSuccess) return e;
        const int blocks = (int)std::min<int64_t>(((int64_t)r.K * r.D + kKmThreads - 1) / kKmThreads, 1024);
        hipLaunchKernelGGL(km_copy_kernel, dim3(blocks), T, 0, st, a, r.centres_in);
    } else {
        hipLaunchKernelGGL(km_seed_first_kernel, dim3(1), T, 0, st, a);
        const int blocks = std::min(s.nruns, 2048);
        for (int j = 1; j < r.K; ++j) {
            hipLaunchKernelGGL(km_seed_dist_kernel, dim3(blocks), T, 0, st, a, j);
            hipLaunchKernelGGL(km_seed_pick_kernel, dim3(1), T, 0, st, a, j);
        }
    }
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const int nct = (r.D + s.DT - 1) / s.DT;
    for (int t = 0; t <= r.max_iter;) {
        for (int c = 0; c < kKmChunk && t <= r.max_iter; ++c, ++t) {
            hipLaunchKernelGGL(assign, dim3(s.G), T, lds_assign, st, a, t);
            if (a.rpc) hipLaunchKernelGGL(km_sums_kernel, dim3(a.P, nct), T, lds_sums, st, a, t);
            hipLaunchKernelGGL(km_combine_kernel, dim3(r.K, s.cy), T, 0, st, a, t);
        }
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        KmState host;
        if (hipError_t e = hipMemcpyAsync(&host, a.w.state, sizeof(host), hipMemcpyDeviceToHost, st);
            e != hipSuccess)
            return e;
        if (hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return e;
        if (host.done[t & 1]) break;
    }
    const int blocks = (int)std::min<int64_t>(((int64_t)r.N + kKmThreads - 1) / kKmThreads, 1024);
    hipLaunchKernelGGL(km_finish_kernel, dim3(blocks), T, 0, st, a);
    return hipGetLastError();
}

}  // namespace psvi
