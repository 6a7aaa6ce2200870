// pool_global.hip -- a pool whose window is the WHOLE (h, w) map: Flux GlobalMaxPool() / GlobalMeanPool(), and AdaptiveMaxPool / AdaptiveMeanPool with output (1, 1) (layer
// kinds 12 / 13 where the resolved geometry has oh = ow = 1: is_global_pool, common.h).  Layout: X[feature][column], features in the internal [c][y][x] order, so a channel's
// map is n = h * w CONTIGUOUS rows and the reduction runs along the strided axis, as in groupnorm.hip.  pool.hip gives such a window one thread per (channel, four columns)
// that walks all n taps serially (and, in the MaxPool backward, re-scans the earlier taps per input element); here a workgroup shares the walk.
//
// Work split (groupnorm.hip's): one workgroup per (column tile, channel); 256 threads = (slot = tid / 16, column piece = tid mod 16).  A piece is four columns as ONE 16-byte
// access where leading dimension, column offset, column count and base pointers allow it (tile = 64 columns: 16 lanes cover a 256-byte row piece), otherwise one column
// (tile = 16 columns: B = 5, where the target pass starts at column 5).  Slot s owns the rows s, s + 16, s + 32, ... of the channel in ascending order; the 16 slot partials
// meet in LDS and every thread combines them in ascending slot order.  Plain vector loads and stores, no float atomics, no counters, no cross-workgroup dependency.
//
// Canonical results (DESIGN.md section 4 "Global and adaptive pool layers"); they depend on n alone -- never on the column count, the column's position, the aligned / unaligned
// path, graph or eager:
//   mean forward    a slot sums its rows as one chain from +0; the 16 slot sums are added in ascending slot order, slot 0 first; y = sum / f32(n).  For n <= 16 every slot
//                   holds at most one row and this IS pool.hip's chain over the taps (the empty slots add +0, which changes no bit of a sum that started from +0)
//   mean backward   dX = dact(dY_c / f32(n), x) for every row of the channel: element-wise, pool.hip's bits at every n
//   max forward     y = the value at the FIRST row, in ascending row order, that holds the maximum; ties are decided by ==, so +0 and -0 tie and the earlier row's bits win:
//                   pool.hip's result bit for bit on NaN-free maps.  (value, row) is carried through the slot walk (a later row replaces only when GREATER) and the LDS
//                   combine (the greater value wins, on equal values the smaller row)
//   max backward    that first row receives dY_c, every other row +0, then the producing layer's activation derivative on that layer's output (= this layer's input), as
//                   pool.hip does.  The row is RECOMPUTED by the backward workgroup from X with the forward's own walk -- nothing is stashed (DESIGN.md says why)
#include "common.h"

#define GP_SLOTS 16
#define GP_UNROLL 4      /* rows a slot has in flight per turn of its walk */

template <int V> struct GpVec { float v[V]; };
template <int V> struct GpRow { int r[V]; };
template <int V> __device__ __forceinline__ GpVec<V> gp_ld(const float* p);
template <> __device__ __forceinline__ GpVec<1> gp_ld<1>(const float* p) { GpVec<1> r; r.v[0] = *p; return r; }
template <> __device__ __forceinline__ GpVec<4> gp_ld<4>(const float* p) { const float4 q = *reinterpret_cast<const float4*>(p); GpVec<4> r; r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w; return r; }
template <int V> __device__ __forceinline__ void gp_st(float* p, const GpVec<V>& a);
template <> __device__ __forceinline__ void gp_st<1>(float* p, const GpVec<1>& a) { *p = a.v[0]; }
template <> __device__ __forceinline__ void gp_st<4>(float* p, const GpVec<4>& a) { *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]); }

#define GP_PROLOGUE(NCOLS) \
    const int tid = threadIdx.x, slot = tid >> 4, cl = (tid & 15) * V; \
    const int c = blockIdx.x * 16 * V + cl, ch = blockIdx.y; \
    const bool live = c < (NCOLS)      /* V == 4: the column count is a multiple of 4, so a live piece is four live columns */

// the channel's sum per column of this thread's piece: xb = the channel's row 0 at this thread's first column.  Called by every thread (barriers)
template <int V> __device__ __forceinline__ GpVec<V> gp_sum(float* red, const float* __restrict__ xb, int ldx, int n, bool live, int slot, int cl) {
    GpVec<V> s;
#pragma unroll
    for (int j = 0; j < V; j++) s.v[j] = 0.0f;
    if (live) {
        int i = slot;
        for (; i + (GP_UNROLL - 1) * GP_SLOTS < n; i += GP_UNROLL * GP_SLOTS) {
            GpVec<V> x[GP_UNROLL];
#pragma unroll
            for (int k = 0; k < GP_UNROLL; k++) x[k] = gp_ld<V>(xb + (size_t)(i + k * GP_SLOTS) * ldx);
#pragma unroll
            for (int k = 0; k < GP_UNROLL; k++) {
#pragma unroll
                for (int j = 0; j < V; j++) s.v[j] += x[k].v[j]; }
        }
        for (; i < n; i += GP_SLOTS) { const GpVec<V> x = gp_ld<V>(xb + (size_t)i * ldx);
#pragma unroll
            for (int j = 0; j < V; j++) s.v[j] += x.v[j]; }
    }
    gp_st<V>(red + slot * 16 * V + cl, s);
    __syncthreads();
    GpVec<V> t = gp_ld<V>(red + cl);
#pragma unroll
    for (int q = 1; q < GP_SLOTS; q++) { const GpVec<V> o = gp_ld<V>(red + q * 16 * V + cl);
#pragma unroll
        for (int j = 0; j < V; j++) t.v[j] += o.v[j]; }
    return t;
}

// the channel's maximum and the FIRST row that holds it, per column of this thread's piece.  A slot without a row (n < 16) carries row = n, which loses every comparison.
// Called by every thread (barriers); red: 16 * 16 * V floats, redr: as many ints
template <int V> __device__ __forceinline__ void gp_first_max(float* red, int* redr, const float* __restrict__ xb, int ldx, int n, bool live, int slot, int cl, GpVec<V>& m, GpRow<V>& r) {
#pragma unroll
    for (int j = 0; j < V; j++) { m.v[j] = 0.0f; r.r[j] = n; }
    if (live && slot < n) {
        m = gp_ld<V>(xb + (size_t)slot * ldx);
#pragma unroll
        for (int j = 0; j < V; j++) r.r[j] = slot;
        int i = slot + GP_SLOTS;
        for (; i + (GP_UNROLL - 1) * GP_SLOTS < n; i += GP_UNROLL * GP_SLOTS) {
            GpVec<V> x[GP_UNROLL];
#pragma unroll
            for (int k = 0; k < GP_UNROLL; k++) x[k] = gp_ld<V>(xb + (size_t)(i + k * GP_SLOTS) * ldx);
#pragma unroll
            for (int k = 0; k < GP_UNROLL; k++) {
#pragma unroll
                for (int j = 0; j < V; j++) if (x[k].v[j] > m.v[j]) { m.v[j] = x[k].v[j]; r.r[j] = i + k * GP_SLOTS; } }
        }
        for (; i < n; i += GP_SLOTS) { const GpVec<V> x = gp_ld<V>(xb + (size_t)i * ldx);
#pragma unroll
            for (int j = 0; j < V; j++) if (x.v[j] > m.v[j]) { m.v[j] = x.v[j]; r.r[j] = i; } }
    }
    gp_st<V>(red + slot * 16 * V + cl, m);
#pragma unroll
    for (int j = 0; j < V; j++) redr[slot * 16 * V + cl + j] = r.r[j];
    __syncthreads();
    m = gp_ld<V>(red + cl);
#pragma unroll
    for (int j = 0; j < V; j++) r.r[j] = redr[cl + j];
#pragma unroll
    for (int q = 1; q < GP_SLOTS; q++) { const GpVec<V> o = gp_ld<V>(red + q * 16 * V + cl);
#pragma unroll
        for (int j = 0; j < V; j++) { const int orow = redr[q * 16 * V + cl + j];
            if (orow < n && (r.r[j] >= n || o.v[j] > m.v[j] || (o.v[j] == m.v[j] && orow < r.r[j]))) { m.v[j] = o.v[j]; r.r[j] = orow; } } }
}

// X[C * n][ldx] read at columns col0 .. col0 + ncols; Y[C][ncols]
template <int V, int MEAN> __global__ __launch_bounds__(256) void k_gpool_fwd(int n, const float* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y) {
    __shared__ __attribute__((aligned(16))) float red[GP_SLOTS * 16 * V];
    __shared__ int redr[MEAN ? 1 : GP_SLOTS * 16 * V];
    GP_PROLOGUE(ncols);
    const float* xb = X + (size_t)ch * n * ldx + col0 + c;
    GpVec<V> y;
    if (MEAN) { y = gp_sum<V>(red, xb, ldx, n, live, slot, cl); const float fn = (float)n;
#pragma unroll
        for (int j = 0; j < V; j++) y.v[j] = y.v[j] / fn; }
    else { GpRow<V> r; gp_first_max<V>(red, redr, xb, ldx, n, live, slot, cl, y, r); }
    if (live && slot == 0) gp_st<V>(Y + (size_t)ch * ncols + c, y);      // no barrier below
}

// dY[C][B]; X[C * n][ld] = the pool's input = the producing layer's output (online net, s columns 0 .. B); dX[C * n][B]
template <int V, int MEAN> __global__ __launch_bounds__(256) void k_gpool_bwd(int n, const float* __restrict__ dY, const float* __restrict__ X, int ld, int B, float* __restrict__ dX, int act_src) {
    __shared__ __attribute__((aligned(16))) float red[MEAN ? 4 : GP_SLOTS * 16 * V];
    __shared__ int redr[MEAN ? 1 : GP_SLOTS * 16 * V];
    GP_PROLOGUE(B);
    const float* xb = X + (size_t)ch * n * ld + c;
    GpVec<V> m; GpRow<V> r;
    if (!MEAN) gp_first_max<V>(red, redr, xb, ld, n, live, slot, cl, m, r);
    if (!live) return;      // no barrier below
    GpVec<V> d = gp_ld<V>(dY + (size_t)ch * B + c);
#pragma unroll
    for (int j = 0; j < V; j++) d.v[j] = 0.0f + d.v[j];      // pool.hip's gather sums the one covering window from +0: a dY of -0 arrives as +0 there, so here too
    if (MEAN) { const float fn = (float)n;
#pragma unroll
        for (int j = 0; j < V; j++) d.v[j] = d.v[j] / fn; }
    float* ob = dX + (size_t)ch * n * B + c;
    int i = slot;
    for (; i + (GP_UNROLL - 1) * GP_SLOTS < n; i += GP_UNROLL * GP_SLOTS) {      // GP_UNROLL rows in flight per turn (element-wise: any order gives the same bits)
        GpVec<V> x[GP_UNROLL];
#pragma unroll
        for (int k = 0; k < GP_UNROLL; k++) x[k] = gp_ld<V>(xb + (size_t)(i + k * GP_SLOTS) * ld);
#pragma unroll
        for (int k = 0; k < GP_UNROLL; k++) { const int row = i + k * GP_SLOTS; GpVec<V> o;
#pragma unroll
            for (int j = 0; j < V; j++) o.v[j] = dact_f(MEAN ? d.v[j] : (r.r[j] == row ? d.v[j] : 0.0f), x[k].v[j], act_src);
            gp_st<V>(ob + (size_t)row * B, o); }
    }
    for (; i < n; i += GP_SLOTS) {
        const GpVec<V> x = gp_ld<V>(xb + (size_t)i * ld); GpVec<V> o;
#pragma unroll
        for (int j = 0; j < V; j++) o.v[j] = dact_f(MEAN ? d.v[j] : (r.r[j] == i ? d.v[j] : 0.0f), x.v[j], act_src);
        gp_st<V>(ob + (size_t)i * B, o);
    }
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static dim3 gp_grid(const LayerDev& L, int ncols, bool vec) { return dim3((unsigned)((ncols + (vec ? 63 : 15)) / (vec ? 64 : 16)), (unsigned)L.cout); }
void launch_gpool_fwd(hipStream_t st, const LayerDev& L, const float* X, int ldx, int col0, int ncols, float* Y) {
    const int n = L.ih * L.iw; const bool mean = is_mean_pool(L.kind);
    const bool vec = ldx % 4 == 0 && col0 % 4 == 0 && ncols % 4 == 0 && al16(X) && al16(Y);
    if (vec && mean) hipLaunchKernelGGL((k_gpool_fwd<4, 1>), gp_grid(L, ncols, true), dim3(256), 0, st, n, X, ldx, col0, ncols, Y);
    else if (vec) hipLaunchKernelGGL((k_gpool_fwd<4, 0>), gp_grid(L, ncols, true), dim3(256), 0, st, n, X, ldx, col0, ncols, Y);
    else if (mean) hipLaunchKernelGGL((k_gpool_fwd<1, 1>), gp_grid(L, ncols, false), dim3(256), 0, st, n, X, ldx, col0, ncols, Y);
    else hipLaunchKernelGGL((k_gpool_fwd<1, 0>), gp_grid(L, ncols, false), dim3(256), 0, st, n, X, ldx, col0, ncols, Y);
}
void launch_gpool_bwd(hipStream_t st, const LayerDev& L, const float* dY, const float* X, int ld, int B, float* dX, int act_src) {
    const int n = L.ih * L.iw; const bool mean = is_mean_pool(L.kind);
    const bool vec = ld % 4 == 0 && B % 4 == 0 && al16(dY) && al16(X) && al16(dX);
    if (vec && mean) hipLaunchKernelGGL((k_gpool_bwd<4, 1>), gp_grid(L, B, true), dim3(256), 0, st, n, dY, X, ld, B, dX, act_src);
    else if (vec) hipLaunchKernelGGL((k_gpool_bwd<4, 0>), gp_grid(L, B, true), dim3(256), 0, st, n, dY, X, ld, B, dX, act_src);
    else if (mean) hipLaunchKernelGGL((k_gpool_bwd<1, 1>), gp_grid(L, B, false), dim3(256), 0, st, n, dY, X, ld, B, dX, act_src);
    else hipLaunchKernelGGL((k_gpool_bwd<1, 0>), gp_grid(L, B, false), dim3(256), 0, st, n, dY, X, ld, B, dX, act_src);
}
