// pool.hip -- Flux MaxPool / MeanPool (pad 0; and the adaptive kinds on their resolved geometry, unless the window is the whole map: pool_global.hip) over the batch-innermost Y[feature][column] layout: parameter-free layers between the
// convolutions of a Q-network.  No contraction, no MFMA: every launch here is bandwidth- and launch-bound.
//
// Canonical order:
//   MaxPool forward   the maximum over the window's taps in (ky, kx) ascending order of the [c][y][x] layout (exact: a tap replaces the running maximum only when it is GREATER)
//   MaxPool backward  a window sends its dY to the FIRST tap, in that order, that holds the maximum.  Nothing is stashed: the tap is recomputed as "x == y and no earlier tap
//                     of the window equals y" (the forward's maximum is one of the taps, bit for bit)
//   MeanPool forward  y = (chain sum of the taps, ascending, from +0) / f32(kh*kw)
//   MeanPool backward (sum of dY over the covering windows) / f32(kh*kw)
//   both backwards    a GATHER per input element over its covering windows in ascending (oy, ox), summed from +0 -- at most ceil(kh/sh) * ceil(kw/sw) of them, no float atomics;
//                     inputs no window covers get 0.  The sum is then multiplied by the producing layer's activation derivative (dact_f on that layer's output = the pool's input),
//                     exactly as a convolution's dX epilogue does.
// Work split: a thread owns (one output feature [forward] or one input feature [backward], four adjacent columns).  Where every row start is 16-byte aligned (leading dimensions,
// column offset and column count all multiples of 4) the four columns are ONE 16-byte access and a wave covers whole 256-byte row pieces; otherwise (B = 5: ten columns, the target
// pass starting at column 5) the thread walks its columns one by one.
#include "common.h"

struct PoolGeo { int C, ih, iw, oh, ow, kh, kw, sh, sw; };
static PoolGeo pool_geo(const LayerDev& L) { PoolGeo g; g.C = L.cin; g.ih = L.ih; g.iw = L.iw; g.oh = L.oh; g.ow = L.ow; g.kh = L.kh; g.kw = L.kw; g.sh = L.sh; g.sw = L.sw; return g; }

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// X[in_feat][ldx] read at columns col0 .. col0 + ncols; Y[out_feat][ncols]
template <int MEAN> __global__ __launch_bounds__(256) void k_pool_fwd(PoolGeo G, const float* __restrict__ X, int ldx, int col0, int ncols, float* __restrict__ Y, int vec) {
    const int ng = (ncols + 3) >> 2;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t f = t / ng; const int c0 = (int)(t - f * ng) * 4;
    const int npos = G.oh * G.ow;
    if (f >= (size_t)G.C * npos) return;
    const int c = (int)(f / npos), pos = (int)(f - (size_t)c * npos), oy = pos / G.ow, ox = pos - oy * G.ow;
    const float* xb = X + ((size_t)(c * G.ih + oy * G.sh) * G.iw + ox * G.sw) * ldx + col0 + c0;
    float* yb = Y + f * ncols + c0;
    const float nwin = (float)(G.kh * G.kw);
    if (vec) {
        float4 m = MEAN ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : ld4(xb);
        for (int ky = 0; ky < G.kh; ky++) for (int kx = 0; kx < G.kw; kx++) {
            const float4 v = ld4(xb + (size_t)(ky * G.iw + kx) * ldx);
            if (MEAN) { m.x += v.x; m.y += v.y; m.z += v.z; m.w += v.w; }
            else { m.x = v.x > m.x ? v.x : m.x; m.y = v.y > m.y ? v.y : m.y; m.z = v.z > m.z ? v.z : m.z; m.w = v.w > m.w ? v.w : m.w; }
        }
        if (MEAN) { m.x /= nwin; m.y /= nwin; m.z /= nwin; m.w /= nwin; }
        *reinterpret_cast<float4*>(yb) = m;
        return;
    }
    const int nj = min(4, ncols - c0);
    for (int j = 0; j < nj; j++) {
        float m = MEAN ? 0.0f : xb[j];
        for (int ky = 0; ky < G.kh; ky++) for (int kx = 0; kx < G.kw; kx++) {
            const float v = xb[(size_t)(ky * G.iw + kx) * ldx + j];
            if (MEAN) m += v; else m = v > m ? v : m;
        }
        yb[j] = MEAN ? m / nwin : m;
    }
}

// dY[out_feat][B]; X[in_feat][ld] = the pool's input = the producing layer's output, Y[out_feat][ld] = the pool's output (online net, s columns 0 .. B); dX[in_feat][B]
template <int MEAN> __global__ __launch_bounds__(256) void k_pool_bwd(PoolGeo G, const float* __restrict__ dY, const float* __restrict__ X, const float* __restrict__ Y, int ld, int B,
                                                                      float* __restrict__ dX, int act_src, int vec) {
    const int ng = (B + 3) >> 2;
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t f = t / ng; const int c0 = (int)(t - f * ng) * 4;
    const int ipos = G.ih * G.iw, npos = G.oh * G.ow;
    if (f >= (size_t)G.C * ipos) return;
    const int c = (int)(f / ipos), p = (int)(f - (size_t)c * ipos), iy = p / G.iw, ix = p - iy * G.iw;
    // the windows that cover (iy, ix): oy * sh <= iy <= oy * sh + kh - 1, clipped to the output map
    const int oy_lo = iy - G.kh + 1 <= 0 ? 0 : (iy - G.kh + G.sh) / G.sh, oy_hi = min(G.oh - 1, iy / G.sh);
    const int ox_lo = ix - G.kw + 1 <= 0 ? 0 : (ix - G.kw + G.sw) / G.sw, ox_hi = min(G.ow - 1, ix / G.sw);
    const float* xrow = X + f * ld + c0;
    const float* xch = X + (size_t)c * ipos * ld + c0;      // channel base, for the earlier taps of a window
    const float nwin = (float)(G.kh * G.kw);
    if (vec) {
        const float4 x = ld4(xrow);
        float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (int oy = oy_lo; oy <= oy_hi; oy++) for (int ox = ox_lo; ox <= ox_hi; ox++) {
            const size_t fo = (size_t)c * npos + oy * G.ow + ox;
            const float4 d = ld4(dY + fo * B + c0);
            if (MEAN) { g.x += d.x; g.y += d.y; g.z += d.z; g.w += d.w; continue; }
            const float4 y = ld4(Y + fo * ld + c0);
            bool hx = x.x == y.x, hy = x.y == y.y, hz = x.z == y.z, hw = x.w == y.w;
            if (hx || hy || hz || hw) {      // first-tap rule: an earlier tap of this window that also holds the maximum takes the gradient instead
                const int ty = iy - oy * G.sh, tx = ix - ox * G.sw;
                for (int ky = 0; ky <= ty; ky++) { const int kxe = ky < ty ? G.kw : tx;
                    for (int kx = 0; kx < kxe; kx++) {
                        const float4 e = ld4(xch + (size_t)((oy * G.sh + ky) * G.iw + ox * G.sw + kx) * ld);
                        hx = hx && !(e.x == y.x); hy = hy && !(e.y == y.y); hz = hz && !(e.z == y.z); hw = hw && !(e.w == y.w);
                    } }
            }
            g.x += hx ? d.x : 0.0f; g.y += hy ? d.y : 0.0f; g.z += hz ? d.z : 0.0f; g.w += hw ? d.w : 0.0f;
        }
        if (MEAN) { g.x /= nwin; g.y /= nwin; g.z /= nwin; g.w /= nwin; }
        dact_v4(g, x, act_src);
        *reinterpret_cast<float4*>(dX + f * B + c0) = g;
        return;
    }
    const int nj = min(4, B - c0);
    for (int j = 0; j < nj; j++) {
        const float x = xrow[j]; float g = 0.0f;
        for (int oy = oy_lo; oy <= oy_hi; oy++) for (int ox = ox_lo; ox <= ox_hi; ox++) {
            const size_t fo = (size_t)c * npos + oy * G.ow + ox;
            const float d = dY[fo * B + c0 + j];
            if (MEAN) { g += d; continue; }
            const float y = Y[fo * ld + c0 + j];
            bool hit = x == y;
            if (hit) {
                const int ty = iy - oy * G.sh, tx = ix - ox * G.sw;
                for (int ky = 0; ky <= ty; ky++) { const int kxe = ky < ty ? G.kw : tx;
                    for (int kx = 0; kx < kxe; kx++) hit = hit && !(xch[(size_t)((oy * G.sh + ky) * G.iw + ox * G.sw + kx) * ld + j] == y); }
            }
            g += hit ? d : 0.0f;
        }
        if (MEAN) g /= nwin;
        dX[f * B + c0 + j] = dact_f(g, x, act_src);
    }
}

static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
void launch_pool_fwd(hipStream_t st, const LayerDev& L, const float* X, int ldx, int col0, int ncols, float* Y) {
    const PoolGeo G = pool_geo(L);
    const int vec = (ldx % 4 == 0 && col0 % 4 == 0 && ncols % 4 == 0 && al16(X) && al16(Y)) ? 1 : 0;
    const size_t threads = (size_t)L.out_feat * ((ncols + 3) / 4); const unsigned blocks = (unsigned)((threads + 255) / 256);
    if (is_mean_pool(L.kind)) hipLaunchKernelGGL(k_pool_fwd<1>, dim3(blocks), dim3(256), 0, st, G, X, ldx, col0, ncols, Y, vec);
    else hipLaunchKernelGGL(k_pool_fwd<0>, dim3(blocks), dim3(256), 0, st, G, X, ldx, col0, ncols, Y, vec);
}
void launch_pool_bwd(hipStream_t st, const LayerDev& L, const float* dY, const float* X, const float* Y, int ld, int B, float* dX, int act_src) {
    const PoolGeo G = pool_geo(L);
    const int vec = (ld % 4 == 0 && B % 4 == 0 && al16(dY) && al16(X) && al16(Y) && al16(dX)) ? 1 : 0;
    const size_t threads = (size_t)L.in_feat * ((B + 3) / 4); const unsigned blocks = (unsigned)((threads + 255) / 256);
    if (is_mean_pool(L.kind)) hipLaunchKernelGGL(k_pool_bwd<1>, dim3(blocks), dim3(256), 0, st, G, dY, X, Y, ld, B, dX, act_src, vec);
    else hipLaunchKernelGGL(k_pool_bwd<0>, dim3(blocks), dim3(256), 0, st, G, dY, X, Y, ld, B, dX, act_src, vec);
}
