// groupnorm.hip -- Flux GroupNorm(chs, G, act; affine = true, track_stats = false, eps) on a (c, h, w) map in the batch-innermost Y[feature][column] layout, features in the
// internal [c][y][x] order: per batch column and group of c / G contiguous channels, over the group's n_g = (c / G) * h * w elements
//     mu = mean(x)   var = mean((x - mu)^2)   r = 1 / sqrt(var + eps)   x_hat = (x - mu) * r   y = act(gamma_ch * x_hat + beta_ch),   ch = row / (h * w)
// (Flux 0.14 `_norm_layer_forward`: eps INSIDE the root -- torch's law, not the sigma + eps of LayerNorm's `normalise`).  fp32 throughout.  A group is n_g CONTIGUOUS rows and
// the reduction runs along the strided axis, as in layernorm.hip; but n_g is 10^2 .. 10^4 here and the column count small (2B, B or T * B), so a group's rows are cut into
// chunks of GN_R = 64 rows (a constant of the kernels, never a function of the batch) and a workgroup owns (column tile, chunk, group): Nature conv1 with G = 4 at B = 32 is
// 4 groups x 50 chunks = 200 workgroups, not one.
//
// Canonical order (DESIGN.md section 4 "GroupNorm layers"); it depends on (n_g, h * w, GN_R) alone -- never on the column count, the column's position, the aligned /
// unaligned path, graph or eager:
//   inside a chunk          chunk k holds the rows k * 64 .. min(n_g, k * 64 + 64) of the group, len_k of them.  Row i of the chunk belongs to slot i mod 16; a slot sums its
//                           rows in ascending i as one chain from +0; the 16 slot sums are added in ascending slot order, slot 0 first.  Two passes inside the chunk:
//                           mean_k = sum / f32(len_k), then M2_k = the fma chain of (x - mean_k)^2 in the same order.
//   across chunks           Chan's pairwise update in ASCENDING chunk order, starting from chunk 0's (len_0, mean_0, M2_0):
//                           n = n_a + len_k;  d = mean_k - mean;  mean = fma(d, len_k / n, mean);  M2 = fma(d * d, n_a * len_k / n, M2 + M2_k);  n_a = n.
//                           Then var = M2 / f32(n_g), r = 1 / sqrt(var + eps), x_hat = (x - mean) * r, y = act(fma(gamma, x_hat, beta)).
//   backward group sums     g = dpre * gamma_ch; per chunk, in the order above, a_k = sum g and b_k = the fma chain of g * x_hat; across chunks plain sums from +0 in ascending chunk
//                           order; ma = a / f32(n_g), mb = b / f32(n_g);  dX = r * fma(-x_hat, mb, g - ma), then the producing layer's activation derivative on that layer's
//                           output (= this layer's input), as the pool and LayerNorm backwards do.
//   dgamma, dbeta           first per row over its B columns: lane l of one wave sums columns l, l + 64, ... ascending as one chain from +0 (dbeta: sum dpre; dgamma: fma chain
//                           dpre * x_hat), the 64 lane sums are combined by the butterfly v += v[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1; then per channel over its h * w row sums:
//                           lane l of one wave sums rows l, l + 64, ... ascending from +0, the same butterfly.  The order depends on (h * w, B) alone.
// Launches: forward = the chunk statistics (mean_k, M2_k) into a workspace, then the normalise pass, whose workgroups each combine their group's few partials themselves
// (redundant and cheap: no grid-wide dependency on the mean, no float atomics, no last-arriver counters, plain vector stores); backward = chunk sums, dX, then the row sums
// of dpre and dpre * x_hat (a wave per row: c * h * w waves, where one workgroup per channel left the launch on c CUs) and their per-channel sums into dgamma / dbeta.
// Work split: 256 threads = (slot = tid / 16, column piece = tid mod 16); a piece is four columns as ONE 16-byte access where leading dimension, column offset and column count
// are multiples of 4 (tile = 64 columns: 16 lanes cover a 256-byte row piece), otherwise one column (tile = 16 columns: B = 5).  Slot sums meet in LDS as in layernorm.hip.
#include "common.h"

#define GN_SLOTS 16
#define GN_RPS (GN_R / GN_SLOTS)      /* rows per slot and chunk */
#define GN_CB 64                      /* chunks whose partials one combine round stages in LDS (gn_reduce_chunks): 32 KB at four columns a thread, 8 KB at one */

template <int V> struct GnVec { float v[V]; };
template <int V> __device__ __forceinline__ GnVec<V> gn_ld(const float* p);
template <> __device__ __forceinline__ GnVec<1> gn_ld<1>(const float* p) { GnVec<1> r; r.v[0] = *p; return r; }
template <> __device__ __forceinline__ GnVec<4> gn_ld<4>(const float* p) { const float4 q = *reinterpret_cast<const float4*>(p); GnVec<4> r; r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w; return r; }
template <int V> __device__ __forceinline__ void gn_st(float* p, const GnVec<V>& a);
template <> __device__ __forceinline__ void gn_st<1>(float* p, const GnVec<1>& a) { *p = a.v[0]; }
template <> __device__ __forceinline__ void gn_st<4>(float* p, const GnVec<4>& a) { *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]); }
template <int V> __device__ __forceinline__ GnVec<V> gn_zero() { GnVec<V> r;
#pragma unroll
    for (int j = 0; j < V; j++) r.v[j] = 0.0f;
    return r; }

// the 16 slot sums of this thread's columns, slot 0 first (every thread of the tile computes the totals of its own columns)
template <int V> __device__ __forceinline__ GnVec<V> gn_combine(float* red, int slot, int cl, const GnVec<V>& mine) {
    __syncthreads();      // the previous round's readers are done
    gn_st<V>(red + slot * 16 * V + cl, mine);
    __syncthreads();
    GnVec<V> t = gn_ld<V>(red + cl);
#pragma unroll
    for (int s = 1; s < GN_SLOTS; s++) { const GnVec<V> o = gn_ld<V>(red + s * 16 * V + cl);
#pragma unroll
        for (int j = 0; j < V; j++) t.v[j] += o.v[j]; }
    return t;
}

// geometry of one workgroup: blockIdx = (column tile, chunk, group)
struct GnGeo { int ng, hw, nch, G; };
#define GN_PROLOGUE(NCOLS) \
    const int tid = threadIdx.x, slot = tid >> 4, cl = (tid & 15) * V; \
    const int c = blockIdx.x * 16 * V + cl, ch = blockIdx.y, grp = blockIdx.z; \
    const bool live = c < (NCOLS);      /* V == 4: the column count is a multiple of 4, so a live piece is four live columns */ \
    const int len = min(GN_R, geo.ng - ch * GN_R), row0 = grp * geo.ng + ch * GN_R

// part[((grp * nch + ch) * 2 + {0: mean, 1: M2}) * ncols + c]
template <int V> __global__ __launch_bounds__(256) void k_gn_stat(GnGeo geo, const float* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float red[GN_SLOTS * 16 * V];
    GN_PROLOGUE(ncols);
    const float* xb = X + col0 + c;
    GnVec<V> x[GN_RPS], s = gn_zero<V>(), q = gn_zero<V>();
    if (live) {
#pragma unroll
        for (int k = 0; k < GN_RPS; k++) { const int i = slot + k * GN_SLOTS; x[k] = i < len ? gn_ld<V>(xb + (size_t)(row0 + i) * ldx) : gn_zero<V>(); }
#pragma unroll
        for (int k = 0; k < GN_RPS; k++) if (slot + k * GN_SLOTS < len) {
#pragma unroll
            for (int j = 0; j < V; j++) s.v[j] += x[k].v[j]; }
    }
    s = gn_combine<V>(red, slot, cl, s);
    const float fl = (float)len;
#pragma unroll
    for (int j = 0; j < V; j++) s.v[j] = s.v[j] / fl;
    if (live) {
#pragma unroll
        for (int k = 0; k < GN_RPS; k++) if (slot + k * GN_SLOTS < len) {
#pragma unroll
            for (int j = 0; j < V; j++) { const float d = x[k].v[j] - s.v[j]; q.v[j] = fmaf(d, d, q.v[j]); } }
    }
    q = gn_combine<V>(red, slot, cl, q);
    if (!live || slot != 0) return;      // no barrier below
    float* pb = part + (size_t)(grp * geo.nch + ch) * 2 * ncols + c;
    gn_st<V>(pb, s); gn_st<V>(pb + ncols, q);
}

// The combine of a group's chunk partials (two floats per chunk and column) by ONE workgroup, for the columns of its tile; called by every thread (barriers).
//   staging   a round takes the chunks k0 .. k0 + GN_CB: slot s fetches the chunks k0 + s, + 16, + 32, + 48 into LDS, so a round costs ONE global round trip however many
//             chunks the group has (a thread that walked the chunks itself waited for one per few chunks: 9 of the 15 us of the normalise launch on Nature conv1 at B = 32)
//   the chain the first 16 * V threads take ONE column each and walk the staged chunks in ascending order (every thread walking its own columns made the launch VALU-bound
//             at B = 512: 50 chunks x two divisions x 3200 workgroups); the weights of Chan's update depend on the chunk alone and come from a table, one thread per chunk
//   result    through LDS to every thread: CHAN: (mu, r = 1 / sqrt(M2 / n_g + eps)); else the two plain sums from +0, each divided by f32(n_g).
// The arithmetic per column is the canonical one of the file header, whichever thread does it.
// comb[(kk * 2 + {0, 1}) * 16 * V + column], kk = chunk - k0; wtab[kk * 2 + {0, 1}] = len_k / n, n_a * len_k / n; res[{0, 1} * 16 * V + column]
template <int V> struct GnLds { float comb[GN_CB * 2 * 16 * V]; float wtab[GN_CB * 2]; float res[2 * 16 * V]; };
template <int V, bool CHAN> __device__ __forceinline__ void gn_reduce_chunks(const GnGeo& geo, const float* __restrict__ pb, int ncols, bool live, int slot, int cl, float eps, GnLds<V>& L,
                                                                             GnVec<V>& o0, GnVec<V>& o1) {
    const int tid = threadIdx.x; const bool mine = tid < 16 * V;
    float s0 = 0.0f, s1 = 0.0f;
    for (int k0 = 0; k0 < geo.nch; k0 += GN_CB) {
        GnVec<V> a[GN_CB / GN_SLOTS], b[GN_CB / GN_SLOTS];
#pragma unroll
        for (int i = 0; i < GN_CB / GN_SLOTS; i++) { const int k = k0 + slot + i * GN_SLOTS; if (live && k < geo.nch) { a[i] = gn_ld<V>(pb + (size_t)k * 2 * ncols); b[i] = gn_ld<V>(pb + (size_t)k * 2 * ncols + ncols); } }
        __syncthreads();      // the previous round's readers are done
#pragma unroll
        for (int i = 0; i < GN_CB / GN_SLOTS; i++) { const int kk = slot + i * GN_SLOTS; if (live && k0 + kk < geo.nch) { gn_st<V>(L.comb + (kk * 2) * 16 * V + cl, a[i]); gn_st<V>(L.comb + (kk * 2 + 1) * 16 * V + cl, b[i]); } }
        if (CHAN && tid < GN_CB && k0 + tid < geo.nch) {      // every chunk in front of chunk k is full: n_a = k * GN_R
            const int k = k0 + tid; const float na = (float)(k * GN_R), nb = (float)min(GN_R, geo.ng - k * GN_R), n = na + nb;
            L.wtab[tid * 2] = nb / n; L.wtab[tid * 2 + 1] = na * nb / n;
        }
        __syncthreads();
        if (mine) {
            const int cnt = min(GN_CB, geo.nch - k0);
            for (int kk = 0; kk < cnt; kk++) {
                const float v0 = L.comb[(kk * 2) * 16 * V + tid], v1 = L.comb[(kk * 2 + 1) * 16 * V + tid];
                if (!CHAN) { s0 += v0; s1 += v1; }
                else if (k0 + kk == 0) { s0 = v0; s1 = v1; }      // chunk 0 starts the chain
                else { const float d = v0 - s0; s0 = fmaf(d, L.wtab[kk * 2], s0); s1 = fmaf(d * d, L.wtab[kk * 2 + 1], s1 + v1); }
            }
        }
    }
    const float fn = (float)geo.ng;
    if (mine) { L.res[tid] = CHAN ? s0 : s0 / fn; L.res[16 * V + tid] = CHAN ? 1.0f / sqrtf(s1 / fn + eps) : s1 / fn; }
    __syncthreads();
    o0 = gn_ld<V>(L.res + cl); o1 = gn_ld<V>(L.res + 16 * V + cl);
}

// Y[c * h * w][ncols]; stat (or null): mu at [grp][c], r at [G + grp][c], leading dimension ncols
template <int V> __global__ __launch_bounds__(256) void k_gn_norm(GnGeo geo, float eps, int act, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  const float* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y,
                                                                  const float* __restrict__ part, float* __restrict__ stat) {
    __shared__ __attribute__((aligned(16))) GnLds<V> lds;
    GN_PROLOGUE(ncols);
    const float* xb = X + col0 + c;
    GnVec<V> x[GN_RPS];      // the rows are on their way while the statistics are combined
    if (live) {
#pragma unroll
        for (int k = 0; k < GN_RPS; k++) { const int i = slot + k * GN_SLOTS; x[k] = i < len ? gn_ld<V>(xb + (size_t)(row0 + i) * ldx) : gn_zero<V>(); }
    }
    GnVec<V> mu, r; gn_reduce_chunks<V, true>(geo, part + (size_t)grp * geo.nch * 2 * ncols + c, ncols, live, slot, cl, eps, lds, mu, r);
    if (!live) return;      // no barrier below
    if (stat && ch == 0 && slot == 0) { gn_st<V>(stat + (size_t)grp * ncols + c, mu); gn_st<V>(stat + (size_t)(geo.G + grp) * ncols + c, r); }
#pragma unroll
    for (int k = 0; k < GN_RPS; k++) {
        const int i = slot + k * GN_SLOTS; if (i >= len) break;
        const int f = row0 + i, cf = f / geo.hw; const float ga = gamma[cf], be = beta[cf]; GnVec<V> y;
#pragma unroll
        for (int j = 0; j < V; j++) { const float xh = (x[k].v[j] - mu.v[j]) * r.v[j]; y.v[j] = act_f(fmaf(ga, xh, be), act); }
        gn_st<V>(Y + (size_t)f * ncols + c, y);
    }
}

// dpre[n][B]; X[n][ld] (columns 0 .. B); stat: mu at [grp][c], r at [G + grp][c], leading dimension ld_stat; part[((grp * nch + ch) * 2 + {0: sum g, 1: sum g x_hat}) * B + c]
template <int V> __global__ __launch_bounds__(256) void k_gn_bwd_sums(GnGeo geo, const float* __restrict__ gamma, const float* __restrict__ dpre, const float* __restrict__ X, int ld,
                                                                      const float* __restrict__ stat, int ld_stat, int B, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float red[GN_SLOTS * 16 * V];
    GN_PROLOGUE(B);
    GnVec<V> a = gn_zero<V>(), b = gn_zero<V>();
    if (live) {
        const GnVec<V> mu = gn_ld<V>(stat + (size_t)grp * ld_stat + c), r = gn_ld<V>(stat + (size_t)(geo.G + grp) * ld_stat + c);
#pragma unroll
        for (int k = 0; k < GN_RPS; k++) {
            const int i = slot + k * GN_SLOTS; if (i >= len) break;
            const int f = row0 + i; const float ga = gamma[f / geo.hw];
            const GnVec<V> x = gn_ld<V>(X + (size_t)f * ld + c), d = gn_ld<V>(dpre + (size_t)f * B + c);
#pragma unroll
            for (int j = 0; j < V; j++) { const float g = d.v[j] * ga, xh = (x.v[j] - mu.v[j]) * r.v[j]; a.v[j] += g; b.v[j] = fmaf(g, xh, b.v[j]); }
        }
    }
    a = gn_combine<V>(red, slot, cl, a);
    b = gn_combine<V>(red, slot, cl, b);
    if (!live || slot != 0) return;      // no barrier below
    float* pb = part + (size_t)(grp * geo.nch + ch) * 2 * B + c;
    gn_st<V>(pb, a); gn_st<V>(pb + B, b);
}

template <int V> __global__ __launch_bounds__(256) void k_gn_bwd_dx(GnGeo geo, const float* __restrict__ gamma, const float* __restrict__ dpre, const float* __restrict__ X, int ld,
                                                                    const float* __restrict__ stat, int ld_stat, int B, const float* __restrict__ part, float* __restrict__ dX, int act_src) {
    __shared__ __attribute__((aligned(16))) GnLds<V> lds;
    GN_PROLOGUE(B);
    GnVec<V> mu = gn_zero<V>(), r = gn_zero<V>(), x[GN_RPS], d[GN_RPS];      // the rows are on their way while the group sums are combined
    if (live) {
        mu = gn_ld<V>(stat + (size_t)grp * ld_stat + c); r = gn_ld<V>(stat + (size_t)(geo.G + grp) * ld_stat + c);
#pragma unroll
        for (int k = 0; k < GN_RPS; k++) { const int i = slot + k * GN_SLOTS;
            x[k] = i < len ? gn_ld<V>(X + (size_t)(row0 + i) * ld + c) : gn_zero<V>(); d[k] = i < len ? gn_ld<V>(dpre + (size_t)(row0 + i) * B + c) : gn_zero<V>(); }
    }
    GnVec<V> ma, mb; gn_reduce_chunks<V, false>(geo, part + (size_t)grp * geo.nch * 2 * B + c, B, live, slot, cl, 0.0f, lds, ma, mb);      // mean g, mean g * x_hat
    if (!live) return;      // no barrier below
#pragma unroll
    for (int k = 0; k < GN_RPS; k++) {
        const int i = slot + k * GN_SLOTS; if (i >= len) break;
        const int f = row0 + i; const float ga = gamma[f / geo.hw]; GnVec<V> o;
#pragma unroll
        for (int j = 0; j < V; j++) {
            const float g = d[k].v[j] * ga, xh = (x[k].v[j] - mu.v[j]) * r.v[j];
            o.v[j] = dact_f(r.v[j] * fmaf(-xh, mb.v[j], g - ma.v[j]), x[k].v[j], act_src);
        }
        gn_st<V>(dX + (size_t)f * B + c, o);
    }
}

// one wave per row f: rowp[f] = sum over the row's B columns of dpre * x_hat, rowp[n + f] = sum of dpre (n = c * h * w rows)
__global__ __launch_bounds__(256) void k_gn_bwd_rows(int n, int hw, int cpg, int G, const float* __restrict__ dpre, const float* __restrict__ X, int ld, const float* __restrict__ stat, int ld_stat, int B,
                                                     float* __restrict__ rowp) {
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= n) return;      // wave-uniform; no barrier in this kernel
    const int grp = (f / hw) / cpg;
    const float *mu = stat + (size_t)grp * ld_stat, *rr = stat + (size_t)(G + grp) * ld_stat;
    float dg = 0.0f, db = 0.0f;
    for (int c = lane; c < B; c += 64) {
        const float d = dpre[(size_t)f * B + c], xh = (X[(size_t)f * ld + c] - mu[c]) * rr[c];
        db += d; dg = fmaf(d, xh, dg);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { dg += __shfl_xor(dg, o, 64); db += __shfl_xor(db, o, 64); }
    if (lane == 0) { rowp[f] = dg; rowp[(size_t)n + f] = db; }
}
// one wave per channel: g_gamma[ch], g_beta[ch] = the sums of the channel's h * w row sums
__global__ __launch_bounds__(256) void k_gn_bwd_par(int c, int hw, const float* __restrict__ rowp, float* __restrict__ g_gamma, float* __restrict__ g_beta) {
    const int lane = threadIdx.x & 63, chn = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chn >= c) return;      // wave-uniform; no barrier in this kernel
    const size_t n = (size_t)c * hw;
    float dg = 0.0f, db = 0.0f;
    for (int i = lane; i < hw; i += 64) { dg += rowp[(size_t)chn * hw + i]; db += rowp[n + (size_t)chn * hw + i]; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) { dg += __shfl_xor(dg, o, 64); db += __shfl_xor(db, o, 64); }
    if (lane == 0) { g_gamma[chn] = dg; g_beta[chn] = db; }
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static GnGeo gn_geo(const LayerDev& L) { GnGeo g; g.G = L.kh; g.hw = L.npos; g.ng = (L.cout / L.kh) * L.npos; g.nch = gn_nchunks(L); return g; }
static dim3 gn_grid(const GnGeo& g, int ncols, bool vec) { return dim3((unsigned)((ncols + (vec ? 63 : 15)) / (vec ? 64 : 16)), (unsigned)g.nch, (unsigned)g.G); }
void launch_gn_stat(hipStream_t st, const LayerDev& L, const float* X, int ldx, int col0, int ncols, float* part) {
    const GnGeo g = gn_geo(L);
    const bool vec = ldx % 4 == 0 && col0 % 4 == 0 && ncols % 4 == 0 && al16(X) && al16(part);
    if (vec) hipLaunchKernelGGL(k_gn_stat<4>, gn_grid(g, ncols, true), dim3(256), 0, st, g, X, ldx, col0, ncols, part);
    else hipLaunchKernelGGL(k_gn_stat<1>, gn_grid(g, ncols, false), dim3(256), 0, st, g, X, ldx, col0, ncols, part);
}
void launch_gn_norm(hipStream_t st, const LayerDev& L, const float* P, const float* X, int ldx, int col0, int ncols, float* Y, const float* part, float* stat) {
    const GnGeo g = gn_geo(L); const float eps = gn_eps(L); const float *gamma = P + L.w_off, *beta = P + L.b_off;
    const bool vec = ldx % 4 == 0 && col0 % 4 == 0 && ncols % 4 == 0 && al16(X) && al16(Y) && al16(part) && (!stat || al16(stat));
    if (vec) hipLaunchKernelGGL(k_gn_norm<4>, gn_grid(g, ncols, true), dim3(256), 0, st, g, eps, L.act, gamma, beta, X, ldx, col0, ncols, Y, part, stat);
    else hipLaunchKernelGGL(k_gn_norm<1>, gn_grid(g, ncols, false), dim3(256), 0, st, g, eps, L.act, gamma, beta, X, ldx, col0, ncols, Y, part, stat);
}
static bool gn_bwd_vec(const float* dpre, const float* X, int ld, const float* stat, int ld_stat, int B, const float* part, const float* dX) {
    return ld % 4 == 0 && ld_stat % 4 == 0 && B % 4 == 0 && al16(dpre) && al16(X) && al16(stat) && al16(part) && al16(dX);
}
void launch_gn_bwd_sums(hipStream_t st, const LayerDev& L, const float* P, const float* dpre, const float* X, int ld, const float* stat, int ld_stat, int B, float* part) {
    const GnGeo g = gn_geo(L); const float* gamma = P + L.w_off;
    if (gn_bwd_vec(dpre, X, ld, stat, ld_stat, B, part, nullptr)) hipLaunchKernelGGL(k_gn_bwd_sums<4>, gn_grid(g, B, true), dim3(256), 0, st, g, gamma, dpre, X, ld, stat, ld_stat, B, part);
    else hipLaunchKernelGGL(k_gn_bwd_sums<1>, gn_grid(g, B, false), dim3(256), 0, st, g, gamma, dpre, X, ld, stat, ld_stat, B, part);
}
void launch_gn_bwd_dx(hipStream_t st, const LayerDev& L, const float* P, const float* dpre, const float* X, int ld, const float* stat, int ld_stat, int B, const float* part, float* dX, int act_src) {
    const GnGeo g = gn_geo(L); const float* gamma = P + L.w_off;
    if (gn_bwd_vec(dpre, X, ld, stat, ld_stat, B, part, dX)) hipLaunchKernelGGL(k_gn_bwd_dx<4>, gn_grid(g, B, true), dim3(256), 0, st, g, gamma, dpre, X, ld, stat, ld_stat, B, part, dX, act_src);
    else hipLaunchKernelGGL(k_gn_bwd_dx<1>, gn_grid(g, B, false), dim3(256), 0, st, g, gamma, dpre, X, ld, stat, ld_stat, B, part, dX, act_src);
}
void launch_gn_bwd_rows(hipStream_t st, const LayerDev& L, const float* dpre, const float* X, int ld, const float* stat, int ld_stat, int B, float* rowp) {
    const int n = L.cout * L.npos;
    hipLaunchKernelGGL(k_gn_bwd_rows, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, n, L.npos, L.cout / L.kh, L.kh, dpre, X, ld, stat, ld_stat, B, rowp);
}
void launch_gn_bwd_par(hipStream_t st, const LayerDev& L, const float* rowp, float* g_gamma, float* g_beta) {
    hipLaunchKernelGGL(k_gn_bwd_par, dim3((unsigned)((L.cout + 3) / 4)), dim3(256), 0, st, L.cout, L.npos, rowp, g_gamma, g_beta);
}
