// gru.hip -- the GRU cell of the recurrent path (Flux 0.14 GRU = Recur(GRUCell); third-party, recalled like the LSTM's):
//   gates in the order r, z, n; gx = Wi*x (3H rows, bias-free, by the ordinary dense kernels over all T*B columns), gh = Wh*h_{t-1}
//   r = sigm(gx_r + gh_r + b_r),  z = sigm(gx_z + gh_z + b_z),  n = tanh(gx_n + r .* gh_n + b_n),  h' = (1 - z) .* n + z .* h_{t-1}
//   (r multiplies Wh_n*h, not h: GRU, not GRUv3).  Trainable state0 h0, broadcast over the batch (Flux.reset!).
// Canonical order, used by EVERY form below (step, sequence, policy step) so that they agree bit for bit:
//   gh_q   = chain_j (+0; j ascending) fma(h_{t-1}[j], Wh[j][q*H + u], .)                      q = r, z, n
//   r_pre  = (gx_r + gh_r) + b_r ;  z_pre = (gx_z + gh_z) + b_z ;  n_pre = (gx_n + (r * gh_n)) + b_n
//   h'     = ((1 - z) * n) + (z * h_{t-1})
//   sigm / tanh through Float64, rounded once (cell.h)
// BPTT per step, dh = (head gradient) + (dh_{t-1} of step t+1):
//   dn = (dh * (1 - z)) * (1 - n*n) ;  dz = ((dh * (h_{t-1} - n)) * z) * (1 - z) ;  dr = ((dn * gh_n) * r) * (1 - r)
//   dGx = [dr; dz; dn]        -> Wi | b dW and the input dX (dense contractions over T*B columns)
//   dGh = [dr; dz; dn * r]    -> Wh dW (X = h_{t-1})
//   dh_{t-1}[j] = (chain_n (+0; n ascending over 3H) fma(dGh[n], Wh[j][n], .)) + (dh[j] * z[j]) ;  dstate0[u] = sum_b (ascending) dh_{-1}[u][b]
#include "cell.h"

// ------------------------------------------------------------------ the GRU cell (cell.h: what a cell struct provides, and the kernels built from it)
// r and z are early; the n thread keeps gh_n in a register and, once r and z are in LDS, finishes n and h'.  BPTT reads back r, z, n, gh_n, h_{t-1} and
// the head gradient, and writes dGh apart from dG; the junk bias row of its Wh dW pass holds sum(dn .* r): cleared.
struct GruCell {
    static constexpr int NG = 3, NE = 2, FIN = 2;
    static constexpr bool HAS_C = false, TWO_DG = true, ADD_DH = true;
    static constexpr size_t SEQ_LDS = 64 * 1024;
    static __device__ __forceinline__ float gate_act(int, float pre) { return sigm_f(pre); }
    static __device__ __forceinline__ CellFwd finish(const float* a, float ghn, float gx, float b, float hp, float, int) {
        const float r = a[0], z = a[1];
        const float rg = r * ghn; const float np_ = (gx + rg) + b; const float n = tanh_f(np_);
        const float omz = 1.0f - z; const float t1 = omz * n; const float t2 = z * hp; const float h = t1 + t2;
        return {h, 0.0f, n, ghn};
    }
    struct St { float r, z, n, ghn, hp, dH; };
    static __device__ __forceinline__ St fetch(const CellBwdArgs& A, int u, size_t k) {
        const int H = A.H, TB = A.TB; St s;
        s.r = A.gates[(size_t)u * TB + k]; s.z = A.gates[(size_t)(H + u) * TB + k]; s.n = A.gates[(size_t)(2 * H + u) * TB + k];
        s.ghn = A.aux[(size_t)u * TB + k]; s.hp = A.hprev[(size_t)u * TB + k]; s.dH = A.dH[(size_t)u * TB + k]; return s;
    }
    static __device__ __forceinline__ float bwd(const St& s, float dhn, float, int, float* dG, float* dGh) {
        const float r = s.r, z = s.z, n = s.n, ghn = s.ghn, hp = s.hp;
        const float dh = s.dH + dhn;
        const float omz = 1.0f - z; const float n2 = n * n; const float omn2 = 1.0f - n2; const float a1 = dh * omz; const float dn = a1 * omn2;
        const float hmn = hp - n; const float b1 = dh * hmn; const float b2 = b1 * z; const float dz = b2 * omz;
        const float c1 = dn * ghn; const float c2 = c1 * r; const float omr = 1.0f - r; const float dr = c2 * omr;
        const float dnr = dn * r;
        dG[0] = dr; dG[1] = dz; dG[2] = dn;
        dGh[0] = dr; dGh[1] = dz; dGh[2] = dnr;
        return dh * z;
    }
};
const CellOps* gru_cell_ops() { static const CellOps ops = cell_ops_entry<GruCell>("gru", "GRU", false, true, launch_cell_seq<GruCell>); return &ops; }
