// lmf.hip — Low-rank Multimodal Fusion (MERBench/toolkit/models/lmf.py:64-86), forward and backward, fp32.
//
//   P_m[r,b,o] = F_m[r,0,o] + sum_k h_m[b,k] F_m[r,k+1,o]          m in {audio, video, text}; the appended one is folded in
//   out[b,o]   = sum_r w[r] P_a[r,b,o] P_v[r,b,o] P_t[r,b,o] + bias[o]
//
// h_m [B,H], F_m [R,H+1,O] (the parameter's own layout), w [R], bias [O], proj = (P_a, P_v, P_t) as [3,R,B,O].
// At the tuning grid's sizes (H <= 256, R <= 6, O <= 128, B = 32) this is <= 38 MFLOP: launch-latency bound, so the forward
// is ONE launch and the backward is ONE launch (four block roles in one grid), neither count depending on B, H, R or O.
// Plain VALU FMAs; F_m is always read along o (coalesced).  No atomics: every sum runs in one fixed order, so two runs give the
// same bits, and a forward row is computed from that row alone with the same instruction sequence wherever it sits in its
// tile (row b has the same bits at any B).
#include "common.h"

namespace mer {

constexpr int LMF_RB = 4;      // forward: rows per block (registers of one thread)
constexpr int LMF_MAXH = 1024, LMF_MAXO = 512, LMF_MAXR = 16, LMF_MAXB = 2048;

// ---------------------------------------------------------------------------------------------------------------------
// forward: block = (64 lanes over o) x (R waves, one per rank), grid = (ceil(O/64), ceil(B/4)).
// LDS: hs [3][H][4] (the tile's rows of the three encoders, row index fastest so that one 16-byte broadcast read feeds
// four FMAs) and zs [R][4][64] (w[r] P_a P_v P_t per rank, summed over r = 0 .. R-1 in that order).
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void lmf_fwd_kernel(const float* __restrict__ ha, const float* __restrict__ hv,
                                                       const float* __restrict__ ht, const float* __restrict__ fa,
                                                       const float* __restrict__ fv, const float* __restrict__ ft,
                                                       const float* __restrict__ w, const float* __restrict__ bias, int B, int H,
                                                       int R, int O, float* __restrict__ proj, float* __restrict__ out) {
  extern __shared__ __align__(16) float lmf_smem[];
  float* hs = lmf_smem;
  float* zs = lmf_smem + 3 * H * LMF_RB;
  const int lane = threadIdx.x, r = threadIdx.y;
  const int tid = r * 64 + lane, nth = 64 * R;
  const int o = blockIdx.x * 64 + lane, b0 = blockIdx.y * LMF_RB;

  for (int i = tid; i < 3 * LMF_RB * H; i += nth) {
    const int m = i / (LMF_RB * H), j = (i / H) % LMF_RB, k = i % H;
    const float* hp = m == 0 ? ha : (m == 1 ? hv : ht);
    const int b = b0 + j;
    hs[(m * H + k) * LMF_RB + j] = b < B ? hp[(long long)b * H + k] : 0.f;
  }
  __syncthreads();

  float z[LMF_RB];
#pragma unroll
  for (int j = 0; j < LMF_RB; ++j) z[j] = 0.f;
  if (o < O) {
    // one k loop for the three modalities, unrolled by 8 so that 24 factor loads are issued per wait (the loop is a chain of L2
    // latencies; unrolling by 16 measured 2x slower); each accumulator still sees k = 0 .. H-1 in order
    const long long fo = (long long)r * (H + 1) * O + o;
    const float* Fa = fa + fo;
    const float* Fv = fv + fo;
    const float* Ft = ft + fo;
    const f32x4* h4a = reinterpret_cast<const f32x4*>(hs);
    const f32x4* h4v = reinterpret_cast<const f32x4*>(hs + H * LMF_RB);
    const f32x4* h4t = reinterpret_cast<const f32x4*>(hs + 2 * H * LMF_RB);
    float p[3][LMF_RB];
    {
      const float a0 = Fa[0], v0 = Fv[0], t0 = Ft[0];
#pragma unroll
      for (int j = 0; j < LMF_RB; ++j) { p[0][j] = a0; p[1][j] = v0; p[2][j] = t0; }
    }
#pragma unroll 8
    for (int k = 0; k < H; ++k) {
      const long long ko = (long long)(k + 1) * O;
      const float xa = Fa[ko], xv = Fv[ko], xt = Ft[ko];
      const f32x4 ya = h4a[k], yv = h4v[k], yt = h4t[k];
#pragma unroll
      for (int j = 0; j < LMF_RB; ++j) {
        p[0][j] = fmaf(ya[j], xa, p[0][j]);
        p[1][j] = fmaf(yv[j], xv, p[1][j]);
        p[2][j] = fmaf(yt[j], xt, p[2][j]);
      }
    }
    if (proj) {
#pragma unroll
      for (int m = 0; m < 3; ++m)
#pragma unroll
        for (int j = 0; j < LMF_RB; ++j)
          if (b0 + j < B) proj[(((long long)m * R + r) * B + (b0 + j)) * O + o] = p[m][j];
    }
    const float wr = w[r];
#pragma unroll
    for (int j = 0; j < LMF_RB; ++j) z[j] = wr * ((p[0][j] * p[1][j]) * p[2][j]);
  }
#pragma unroll
  for (int j = 0; j < LMF_RB; ++j) zs[(r * LMF_RB + j) * 64 + lane] = z[j];
  __syncthreads();
  for (int i = tid; i < LMF_RB * 64; i += nth) {
    const int j = i / 64, l = i % 64;
    const int oo = blockIdx.x * 64 + l, b = b0 + j;
    if (oo < O && b < B) {
      float s = zs[j * 64 + l];
      for (int rr = 1; rr < R; ++rr) s += zs[(rr * LMF_RB + j) * 64 + l];
      out[(long long)b * O + oo] = s + bias[oo];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// backward: one launch of 256-thread blocks, four roles laid end to end in the 1-D grid.
//   dP_m[r,b,o] = dout[b,o] w[r] prod_{n != m} P_n[r,b,o]                            (recomputed from proj by whoever needs it)
//   A  dF_m[r,k',o] = sum_b h'_m[b,k'] dP_m[r,b,o],  h' = [1, h]    block = (m, r, 64 o, 32 k'); b in ascending order
//   B  dh_m[b,k]    = sum_r sum_o dP_m[r,b,o] F_m[r,k+1,o]          block = (m, 16 rows, 64 k); (r, o) in ascending order
//   C  dw[r]        = sum_{b,o} dout[b,o] P_a P_v P_t               block = r; strided partial sums + a fixed LDS tree
//   D  dbias[o]     = sum_b dout[b,o]                               block = 64 o; four strided partial sums over b, added in order
// ---------------------------------------------------------------------------------------------------------------------
struct LmfBwdArgs {
  const float* dout; const float* h[3]; const float* f[3]; const float* w; const float* proj;
  float* dh[3]; float* df[3]; float* dw; float* dbias;
  int B, H, R, O;
  int nOT, nKT, nKH, nBT;      // tiles: o (64), k' of dF (32), k of dh (64), rows of dh (16)
  int nA, nB, nC;              // blocks of roles A, B, C (role D takes the rest)
};

__device__ __forceinline__ float lmf_dp(const LmfBwdArgs& a, int m, int r, int b, int o) {
  const long long plane = (long long)a.R * a.B * a.O;
  const long long i = ((long long)r * a.B + b) * a.O + o;
  const float g = a.dout[(long long)b * a.O + o] * a.w[r];
  const float x = a.proj[(m == 0 ? 1 : 0) * plane + i], y = a.proj[(m == 2 ? 1 : 2) * plane + i];
  return g * (x * y);
}

// role B's operands of one (r, o chunk) iteration into registers: fr = the F_m tile [64 k][64 o] (thread t-th element i = tid + 256 t
// -> k = i / 64, o = i % 64: coalesced along o), dr = dP_m [16 b][64 o]; zeros outside the tensors
__device__ __forceinline__ void lmf_dh_load(const LmfBwdArgs& a, int m, int r, int oc, int kt, int bt, int tid, float (&fr)[16],
                                            float (&dr)[4]) {
  const float* F = a.f[m];
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const int i = tid + 256 * t, k = kt * 64 + (i >> 6), o = oc + (i & 63);
    fr[t] = (k < a.H && o < a.O) ? F[((long long)r * (a.H + 1) + (k + 1)) * a.O + o] : 0.f;
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int i = tid + 256 * t, b = bt * 16 + (i >> 6), o = oc + (i & 63);
    dr[t] = (b < a.B && o < a.O) ? lmf_dp(a, m, r, b, o) : 0.f;
  }
}

__global__ __launch_bounds__(256) void lmf_bwd_kernel(const LmfBwdArgs a) {
  __shared__ __align__(16) float s0[64 * 65];   // A: dP [32 b][64 o];   B: F tile [64 k][65];   C: the reduction tree
  __shared__ __align__(16) float s1[32 * 32];   // A: h' [32 b][32 k'];  B: dP [64 o][16 b]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int B = a.B, H = a.H, R = a.R, O = a.O;
  int blk = blockIdx.x;

  if (blk < a.nA) {   // ---- role A: factor gradients
    const int kt = blk % a.nKT, ot = (blk / a.nKT) % a.nOT, r = (blk / (a.nKT * a.nOT)) % R, m = blk / (a.nKT * a.nOT * R);
    const float* hp = a.h[m];
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int bc = 0; bc < B; bc += 32) {
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        const int i = tid + 256 * t, bb = i >> 6, l = i & 63;
        const int b = bc + bb, o = ot * 64 + l;
        s0[i] = (b < B && o < O) ? lmf_dp(a, m, r, b, o) : 0.f;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = tid + 256 * t, bb = i >> 5, kk = i & 31;
        const int b = bc + bb, k = kt * 32 + kk;
        s1[i] = (b < B && k <= H) ? (k == 0 ? 1.f : hp[(long long)b * H + (k - 1)]) : 0.f;
      }
      __syncthreads();
#pragma unroll 4
      for (int bb = 0; bb < 32; ++bb) {
        const float d = s0[bb * 64 + lane];
        const f32x4 h0 = *reinterpret_cast<const f32x4*>(&s1[bb * 32 + wave * 8]);
        const f32x4 h1 = *reinterpret_cast<const f32x4*>(&s1[bb * 32 + wave * 8 + 4]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          acc[j] = fmaf(h0[j], d, acc[j]);
          acc[4 + j] = fmaf(h1[j], d, acc[4 + j]);
        }
      }
    }
    const int o = ot * 64 + lane;
    if (o < O) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = kt * 32 + wave * 8 + j;
        if (k <= H) a.df[m][((long long)r * (H + 1) + k) * O + o] = acc[j];
      }
    }
    return;
  }
  blk -= a.nA;

  if (blk < a.nB) {   // ---- role B: encoder-output gradients
    const int kt = blk % a.nKH, bt = (blk / a.nKH) % a.nBT, m = blk / (a.nKH * a.nBT);
    float* dh = a.dh[m];
    if (!dh) return;   // (uniform over the block, before any barrier)
    // iterations over (r, 64-wide o chunk) in ascending order; the global loads of iteration it + 1 are issued before the FMAs of
    // iteration it and land in registers meanwhile (the chain of L2 latencies was the whole cost of this role)
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float fr[16], dr[4];
    const int nOC = a.nOT, nIt = R * nOC;
    lmf_dh_load(a, m, 0, 0, kt, bt, tid, fr, dr);
    for (int it = 0; it < nIt; ++it) {
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int i = tid + 256 * t;
        s0[(i >> 6) * 65 + (i & 63)] = fr[t];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int i = tid + 256 * t;
        s1[(i & 63) * 16 + (i >> 6)] = dr[t];
      }
      __syncthreads();
      if (it + 1 < nIt) lmf_dh_load(a, m, (it + 1) / nOC, ((it + 1) % nOC) * 64, kt, bt, tid, fr, dr);
#pragma unroll 8
      for (int oo = 0; oo < 64; ++oo) {
        const float f = s0[lane * 65 + oo];
        const f32x4 d = *reinterpret_cast<const f32x4*>(&s1[oo * 16 + wave * 4]);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(d[j], f, acc[j]);
      }
    }
    const int k = kt * 64 + lane;
    if (k < H) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int b = bt * 16 + wave * 4 + j;
        if (b < B) dh[(long long)b * H + k] = acc[j];
      }
    }
    return;
  }
  blk -= a.nB;

  if (blk < a.nC) {   // ---- role C: fusion-weight gradient, one block per rank
    const int r = blk;
    const long long n = (long long)B * O, plane = (long long)R * n;
    const float* pa = a.proj + (long long)r * n;
    float s = 0.f;
#pragma unroll 4
    for (long long i = tid; i < n; i += 256) s = fmaf(a.dout[i], (pa[i] * pa[plane + i]) * pa[2 * plane + i], s);
    s0[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (tid < st) s0[tid] += s0[tid + st];
      __syncthreads();
    }
    if (tid == 0) a.dw[r] = s0[0];
    return;
  }
  blk -= a.nC;

  {                   // ---- role D: bias gradient, 64 columns per block; rows b = q, q + 4, ... per quarter q, quarters summed in order
    const int o = blk * 64 + lane;
    float s = 0.f;
    if (o < O) {
#pragma unroll 8
      for (int b = wave; b < B; b += 4) s += a.dout[(long long)b * O + o];
    }
    s0[tid] = s;
    __syncthreads();
    if (wave == 0 && o < O) a.dbias[o] = (s0[lane] + s0[64 + lane]) + (s0[128 + lane] + s0[192 + lane]);
  }
}

// Shape check shared by the three entry points; touches no GPU.
static int lmf_check(const char* fn, int B, int H, int R, int O) {
  MER_REQUIRE(H >= 1 && H <= LMF_MAXH, MER_ESHAPE, "%s: H = %d, 1..%d are built", fn, H, LMF_MAXH);
  MER_REQUIRE(O >= 1 && O <= LMF_MAXO, MER_ESHAPE, "%s: O = %d, 1..%d are built", fn, O, LMF_MAXO);
  MER_REQUIRE(R >= 1 && R <= LMF_MAXR, MER_ESHAPE, "%s: R = %d, 1..%d are built", fn, R, LMF_MAXR);
  MER_REQUIRE(B >= 1 && B <= LMF_MAXB, MER_ESHAPE, "%s: B = %d, 1..%d are built", fn, B, LMF_MAXB);
  return MER_OK;
}

}  // namespace mer

using namespace mer;

extern "C" long long mer_lmf_workspace_bytes(int B, int H, int R, int O) {
  const int rc = lmf_check("mer_lmf_workspace_bytes", B, H, R, O);
  return rc != MER_OK ? rc : 0;   // neither direction needs scratch: every reduction finishes inside one block
}

extern "C" int mer_lmf_fwd(const float* ha, const float* hv, const float* ht, const float* fa, const float* fv, const float* ft,
                           const float* w, const float* bias, int B, int H, int R, int O, float* proj, float* out,
                           mer_stream_t stream) {
  const int rc = lmf_check("mer_lmf_fwd", B, H, R, O);
  if (rc != MER_OK) return rc;
  MER_REQUIRE(ha && hv && ht && fa && fv && ft && w && bias && out, MER_EINVAL, "mer_lmf_fwd: null pointer");
  const size_t lds = (size_t)(3 * H * LMF_RB + R * LMF_RB * 64) * sizeof(float);   // <= 64 KiB at H = 1024, R = 16
  hipLaunchKernelGGL(lmf_fwd_kernel, dim3((unsigned)cdiv(O, 64), (unsigned)cdiv(B, LMF_RB)), dim3(64, R), lds, (hipStream_t)stream,
                     ha, hv, ht, fa, fv, ft, w, bias, B, H, R, O, proj, out);
  return check_launch("lmf_fwd");
}

extern "C" int mer_lmf_bwd(const float* dout, const float* ha, const float* hv, const float* ht, const float* fa, const float* fv,
                           const float* ft, const float* w, const float* proj, int B, int H, int R, int O, float* dha, float* dhv,
                           float* dht, float* dfa, float* dfv, float* dft, float* dw, float* dbias, void* workspace,
                           long long workspace_bytes, mer_stream_t stream) {
  const int rc = lmf_check("mer_lmf_bwd", B, H, R, O);
  if (rc != MER_OK) return rc;
  MER_REQUIRE(dout && ha && hv && ht && fa && fv && ft && w && proj, MER_EINVAL, "mer_lmf_bwd: null input pointer");
  MER_REQUIRE(dfa && dfv && dft && dw && dbias, MER_EINVAL, "mer_lmf_bwd: null gradient pointer (only dha / dhv / dht may be null)");
  MER_REQUIRE(workspace_bytes >= 0, MER_EINVAL, "mer_lmf_bwd: workspace_bytes = %lld", workspace_bytes);
  (void)workspace;
  LmfBwdArgs a;
  a.dout = dout; a.w = w; a.proj = proj; a.dw = dw; a.dbias = dbias;
  a.h[0] = ha; a.h[1] = hv; a.h[2] = ht;
  a.f[0] = fa; a.f[1] = fv; a.f[2] = ft;
  a.dh[0] = dha; a.dh[1] = dhv; a.dh[2] = dht;
  a.df[0] = dfa; a.df[1] = dfv; a.df[2] = dft;
  a.B = B; a.H = H; a.R = R; a.O = O;
  a.nOT = (int)cdiv(O, 64); a.nKT = (int)cdiv(H + 1, 32); a.nKH = (int)cdiv(H, 64); a.nBT = (int)cdiv(B, 16);
  a.nA = 3 * R * a.nOT * a.nKT;   // <= 3 * 16 * 8 * 33
  a.nB = 3 * a.nKH * a.nBT;       // <= 3 * 16 * 128
  a.nC = R;
  const int nD = (int)cdiv(O, 64);
  hipLaunchKernelGGL(lmf_bwd_kernel, dim3((unsigned)(a.nA + a.nB + a.nC + nD)), dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("lmf_bwd");
}
