// fusion_group.hip — one training (or evaluation) step for a GROUP of G independent Attention fusion models of one
// architecture (MERBench/toolkit/models/attention.py:36-57 with feat_type 'utt', both heads; main-release.py:31-66):
// the 5 folds of a cross-validation run times N hyper-parameter trials.  The model index is a grid axis of every launch,
// so the number of launches per step does not depend on G; every stage is an ordinary launch on one stream (no
// inter-workgroup communication), and a step allocates nothing and never synchronises (graph-capturable).
//
// Arithmetic contract: each stage is the per-element arithmetic of the single-model kernels (gemm32.hip's MFMA k
// grouping and epilogue, fusion.hip's fuse / CE / MSE / Adam), with the row count of a model (n_g <= B) taking the place
// of the minibatch size.  So model g's losses, outputs, gradients and parameters are bitwise those of a group holding g
// alone, and at dropout 0 bitwise those of FusionGraphTrainer on the same minibatches.  A model with n_g = 0 is idle:
// its parameters, gradients, Adam moments and step counter are not touched.
//
// Dropout keep mask (stateless, counter-based; site 0/1/2 = audio/text/video encoder input, 3 = attention_mlp input):
//   ctr  = (uint64(uint32(step)) << 32) | (site << 30) | (row << 16) | col        (row < 2^14, col < 2^16)
//   z    = seed + (ctr + 1) * 0x9E3779B97F4A7C15                                 (mod 2^64)
//   z    = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31   (splitmix64)
//   u    = float(z >> 40) * 2^-24;   keep = u >= p;   out = keep ? x * (1.0f / (1.0f - p)) : 0      (fp32)
// step is the model's optimiser step counter before the step, row the row within the minibatch.
#include "common.h"

namespace mer {

#define FG_MAXP 16

struct FgCtx {
  const int* cursor;
  const int* count;
  int G, B, S;
};

// rows of model g in the current step (0 = idle; also 0 once the cursor ran past the step table)
__device__ __forceinline__ int fg_rows(const FgCtx& c, int g) {
  const int s = c.cursor ? *c.cursor : 0;
  if (s < 0 || s >= c.S) return 0;
  const int n = c.count[(long long)s * c.G + g];
  return n < 0 ? 0 : (n > c.B ? c.B : n);
}
__device__ __forceinline__ long long fg_slot(const FgCtx& c, int g) {
  return (long long)(c.cursor ? *c.cursor : 0) * c.G + g;
}

__host__ __device__ __forceinline__ uint64_t fg_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ bool fg_keep(uint64_t seed, int step, int site, int row, int col, float p) {
  const uint64_t ctr = ((uint64_t)(uint32_t)step << 32) | ((uint64_t)site << 30) | ((uint64_t)row << 16) | (uint64_t)col;
  const uint64_t z = fg_mix(seed + (ctr + 1ull) * 0x9E3779B97F4A7C15ull);
  return (float)(z >> 40) * (1.0f / 16777216.0f) >= p;
}

// ---- row gather (+ inverted dropout of the three encoder inputs on train steps).  grid (B, G) ----
__global__ __launch_bounds__(256) void fg_gather_kernel(FgCtx c, const float* __restrict__ fa, const float* __restrict__ ft,
                                                        const float* __restrict__ fv, const int* __restrict__ emo_tab,
                                                        const float* __restrict__ val_tab, long long n_rows, const int* __restrict__ index,
                                                        int Da, int Dt, int Dv, float* ws, long long ws_gs, long long o_xa, long long o_xt,
                                                        long long o_xv, long long o_emo, long long o_val, int train,
                                                        const float* __restrict__ drop, const uint64_t* __restrict__ seed,
                                                        const int* __restrict__ step) {
  const int r = blockIdx.x, g = blockIdx.y;
  if (r >= fg_rows(c, g)) return;
  const long long src = index[fg_slot(c, g) * c.B + r];
  const bool ok = src >= 0 && src < n_rows;
  float* w = ws + g * ws_gs;
  const float p = train ? drop[g] : 0.f;
  const float scale = 1.0f / (1.0f - p);
  const uint64_t sd = seed ? seed[g] : 0ull;
  const int st = train ? step[g] : 0;
  for (int e = 0; e < 3; ++e) {
    const int D = e == 0 ? Da : (e == 1 ? Dt : Dv);
    const float* tab = e == 0 ? fa : (e == 1 ? ft : fv);
    float* dst = w + (e == 0 ? o_xa : (e == 1 ? o_xt : o_xv)) + (long long)r * D;
    for (int j = threadIdx.x; j < D; j += blockDim.x) {
      const float x = ok ? tab[src * D + j] : 0.f;
      dst[j] = p > 0.f ? (fg_keep(sd, st, e, r, j, p) ? x * scale : 0.f) : x;
    }
  }
  if (threadIdx.x == 0) {
    reinterpret_cast<int*>(w + o_emo)[r] = ok ? emo_tab[src] : 0;
    w[o_val + r] = ok ? val_tab[src] : 0.f;
  }
}

// ---- grouped exact-fp32 GEMM: gemm32.hip's tile (v_mfma_f32_16x16x4f32, same k grouping and epilogue) over a list of
// problems; grid (sum of the problems' tiles, G).  rows == 1: M is the model's row count (forward, dX); rows == 2: K is (dW).
// gate != NULL folds relu_bwd into the store: v = gate[row, col] > 0 ? v : 0. ----
struct FgGemm {
  const float* a; const float* w; const float* bias; const float* gate; float* c;
  long long lda, ldw, ldc, ldg;
  long long a_gs, w_gs, bias_gs, gate_gs, c_gs;
  int M, N, K, rows, act, accumulate, tiles_n, tile0;
};
struct FgGemmList {
  FgGemm p[FG_MAXP];
  int np;
};

template <bool TA, bool TW>
__global__ __launch_bounds__(64) void fg_gemm_kernel(FgCtx ctx, const FgGemmList L) {
  const int g = blockIdx.y;
  const int ng = fg_rows(ctx, g);
  if (ng == 0) return;
  int pi = 0;
  for (int i = 1; i < L.np; ++i)
    if ((int)blockIdx.x >= L.p[i].tile0) pi = i;
  const FgGemm& P = L.p[pi];
  const int t = (int)blockIdx.x - P.tile0;
  const int tn = t % P.tiles_n, tm = t / P.tiles_n;
  const int M = P.rows == 1 ? ng : P.M, N = P.N, K = P.rows == 2 ? ng : P.K;
  if (tm * 16 >= M) return;
  const float* __restrict__ a = P.a + g * P.a_gs;
  const float* __restrict__ w = P.w + g * P.w_gs;
  const float* bias = P.bias ? P.bias + g * P.bias_gs : nullptr;
  const float* gate = P.gate ? P.gate + g * P.gate_gs : nullptr;
  float* c = P.c + g * P.c_gs;
  const long long lda = P.lda, ldw = P.ldw, ldc = P.ldc;
  const int lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
  const int m = tm * 16 + li;
  const int n = tn * 16 + li;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  const bool va = !TA && (lda % 4 == 0) && ((((uintptr_t)a) & 15) == 0) && (K % 16 == 0) && m < M;
  const bool vw = !TW && (ldw % 4 == 0) && ((((uintptr_t)w) & 15) == 0) && (K % 16 == 0) && n < N;
  for (int k0 = 0; k0 < K; k0 += 16) {
    float av[4], wv[4];
    const int kb = k0 + lg * 4;
    if (va) {
      const f32x4 tt = *reinterpret_cast<const f32x4*>(a + (long long)m * lda + kb);
      av[0] = tt[0]; av[1] = tt[1]; av[2] = tt[2]; av[3] = tt[3];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = kb + j;
        av[j] = (k < K && m < M) ? (TA ? a[(long long)k * lda + m] : a[(long long)m * lda + k]) : 0.f;
      }
    }
    if (vw) {
      const f32x4 tt = *reinterpret_cast<const f32x4*>(w + (long long)n * ldw + kb);
      wv[0] = tt[0]; wv[1] = tt[1]; wv[2] = tt[2]; wv[3] = tt[3];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = kb + j;
        wv[j] = (k < K && n < N) ? (TW ? w[(long long)k * ldw + n] : w[(long long)n * ldw + k]) : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j], wv[j], acc, 0, 0, 0);
  }
  const int col = tn * 16 + li;
  if (col >= N) return;
  const float bv = bias ? bias[col] : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = tm * 16 + lg * 4 + r;
    if (row < M) {
      float v = act_apply(acc[r] + bv, P.act);
      if (gate) v = gate[(long long)row * P.ldg + col] > 0.f ? v : 0.f;
      float* dst = c + (long long)row * ldc + col;
      *dst = P.accumulate ? *dst + v : v;
    }
  }
}

// ---- attention_mlp input dropout (site 3).  grid (B, G) ----
__global__ __launch_bounds__(256) void fg_dropout_kernel(FgCtx c, float* ws, long long ws_gs, long long o_x, long long o_y, int W,
                                                         const float* __restrict__ drop, const uint64_t* __restrict__ seed,
                                                         const int* __restrict__ step, int site) {
  const int r = blockIdx.x, g = blockIdx.y;
  if (r >= fg_rows(c, g)) return;
  const float* x = ws + g * ws_gs + o_x + (long long)r * W;
  float* y = ws + g * ws_gs + o_y + (long long)r * W;
  const float p = drop[g];
  const float scale = 1.0f / (1.0f - p);
  const uint64_t sd = seed ? seed[g] : 0ull;
  const int st = step[g];
  for (int j = threadIdx.x; j < W; j += blockDim.x)
    y[j] = p > 0.f ? (fg_keep(sd, st, site, r, j, p) ? x[j] * scale : 0.f) : x[j];
}

// ---- fuse_fwd: feat[b,j] = sum_e mh[b, e*H + j] * att[b,e] (fmaf chain, e in order).  grid (B, G) ----
__global__ __launch_bounds__(256) void fg_fuse_fwd_kernel(FgCtx c, float* ws, long long ws_gs, long long o_h, long long o_att,
                                                          long long o_out, int H) {
  const int b = blockIdx.x, g = blockIdx.y;
  if (b >= fg_rows(c, g)) return;
  const float* h = ws + g * ws_gs + o_h;
  const float* att = ws + g * ws_gs + o_att;
  float* out = ws + g * ws_gs + o_out;
  const int E = 3;
  for (int j = threadIdx.x; j < H; j += blockDim.x) {
    float s = 0.f;
    for (int e = 0; e < E; ++e) s = fmaf(h[(long long)b * E * H + e * H + j], att[b * E + e], s);
    out[(long long)b * H + j] = s;
  }
}

// ---- fuse_bwd: dh[b,e*H+j] = dout[b,j]*att[b,e]; datt[b,e] = wave_sum of dout*h (fusion.hip's lane split).  grid (3B, G) ----
__global__ __launch_bounds__(64) void fg_fuse_bwd_kernel(FgCtx c, float* ws, long long ws_gs, long long o_dout, long long o_h,
                                                         long long o_att, long long o_dh, long long o_datt, int H) {
  const int E = 3;
  const int b = blockIdx.x / E, e = blockIdx.x % E, g = blockIdx.y, lane = threadIdx.x;
  if (b >= fg_rows(c, g)) return;
  float* base = ws + g * ws_gs;
  const float* dout = base + o_dout;
  const float* h = base + o_h;
  const float a = base[o_att + b * E + e];
  float* dh = base + o_dh;
  float s = 0.f;
  for (int j = lane; j < H; j += 64) {
    const float gr = dout[(long long)b * H + j];
    const long long o = (long long)b * E * H + e * H + j;
    dh[o] = gr * a;
    s = fmaf(gr, h[o], s);
  }
  s = wave_sum(s);
  if (lane == 0) base[o_datt + b * E + e] = s;
}

// ---- CE + MSE rows, their means in row order, the step loss, the outputs into the epoch buffers and (train) the
// loss gradients.  One workgroup of 4 waves per model; CE rows one wave each (fusion.hip's ce_rows lane split). ----
#define FG_MAXB 2048
__global__ __launch_bounds__(256) void fg_loss_kernel(FgCtx c, float* ws, long long ws_gs, long long o_eo, long long o_vo,
                                                      long long o_emo, long long o_val, long long o_demo, long long o_dval, int C1,
                                                      int train, float* out_loss, float* out_emo, float* out_val) {
  __shared__ float ce_row[FG_MAXB];
  __shared__ float mse_row[FG_MAXB];
  const int g = blockIdx.x;
  const int n = fg_rows(c, g);
  if (n == 0) return;
  float* base = ws + g * ws_gs;
  const float* lg = base + o_eo;
  const float* vo = base + o_vo;
  const int* tg = reinterpret_cast<const int*>(base + o_emo);
  const float* vl = base + o_val;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int b = wave; b < n; b += 4) {
    float mx = -INFINITY;
    for (int k = lane; k < C1; k += 64) mx = fmaxf(mx, lg[(long long)b * C1 + k]);
    mx = wave_max(mx);
    float s = 0.f;
    for (int k = lane; k < C1; k += 64) s += expf(lg[(long long)b * C1 + k] - mx);
    s = wave_sum(s);
    const float lse = mx + logf(s);
    const int t = tg[b];
    if (train) {
      for (int k = lane; k < C1; k += 64) {
        const float pr = expf(lg[(long long)b * C1 + k] - lse);
        base[o_demo + (long long)b * C1 + k] = 1.0f * (pr - (k == t ? 1.f : 0.f)) / (float)n;
      }
    }
    if (lane == 0) ce_row[b] = lse - lg[(long long)b * C1 + t];
  }
  for (int b = threadIdx.x; b < n; b += blockDim.x) {
    const float d = vo[b] - vl[b];
    mse_row[b] = d * d;
    if (train) base[o_dval + b] = 2.f * (vo[b] - vl[b]) / (float)n;
  }
  const long long slot = fg_slot(c, g);
  if (out_emo)
    for (int i = threadIdx.x; i < n * C1; i += blockDim.x) out_emo[slot * c.B * C1 + i] = lg[i];
  if (out_val)
    for (int b = threadIdx.x; b < n; b += blockDim.x) out_val[slot * c.B + b] = vo[b];
  __syncthreads();
  if (threadIdx.x == 0 && out_loss) {
    float s = 0.f;
    for (int b = 0; b < n; ++b) s += ce_row[b];
    const float ce = s / (float)n;
    s = 0.f;
    for (int b = 0; b < n; ++b) s += mse_row[b];
    const float mse = s / (float)n;
    out_loss[slot] = ce + mse;
  }
}

// ---- encoders' L3 gradient: dz[b,c] = mh[b,c] > 0 ? dh_fuse[b,c] + dropout_bwd(dx_att1)[b,c] : 0.  grid (B, G) ----
__global__ __launch_bounds__(256) void fg_mh_bwd_kernel(FgCtx c, float* ws, long long ws_gs, long long o_mh, long long o_dhf,
                                                        long long o_dxa, long long o_dz, int W, const float* __restrict__ drop,
                                                        const uint64_t* __restrict__ seed, const int* __restrict__ step, int site) {
  const int r = blockIdx.x, g = blockIdx.y;
  if (r >= fg_rows(c, g)) return;
  float* base = ws + g * ws_gs;
  const long long o = (long long)r * W;
  const float p = drop[g];
  const float scale = 1.0f / (1.0f - p);
  const uint64_t sd = seed ? seed[g] : 0ull;
  const int st = step[g];
  for (int j = threadIdx.x; j < W; j += blockDim.x) {
    const float dx = base[o_dxa + o + j];
    const float dd = p > 0.f ? (fg_keep(sd, st, site, r, j, p) ? dx * scale : 0.f) : dx;
    const float dy = base[o_dhf + o + j] + dd;
    base[o_dz + o + j] = base[o_mh + o + j] > 0.f ? dy : 0.f;
  }
}

// ---- bias gradients: out[n] = sum over the model's rows of x[m, n], rows in order.  grid (sum of 64-column blocks, G) ----
struct FgSum {
  const float* x; float* out;
  long long ldx, x_gs, out_gs;
  int N, blk0;
};
struct FgSumList {
  FgSum p[FG_MAXP];
  int np;
};
__global__ __launch_bounds__(64) void fg_colsum_kernel(FgCtx ctx, const FgSumList L) {
  const int g = blockIdx.y;
  const int M = fg_rows(ctx, g);
  if (M == 0) return;
  int pi = 0;
  for (int i = 1; i < L.np; ++i)
    if ((int)blockIdx.x >= L.p[i].blk0) pi = i;
  const FgSum& P = L.p[pi];
  const int n = ((int)blockIdx.x - P.blk0) * 64 + threadIdx.x;
  if (n >= P.N) return;
  const float* x = P.x + g * P.x_gs;
  float s = 0.f;
  for (int m = 0; m < M; ++m) s += x[(long long)m * P.ldx + n];
  P.out[g * P.out_gs + n] = s;
}

// ---- Adam (fusion.hip adam_dev_kernel's arithmetic) with per-model lr / weight decay / clip.  grid (blocks, G) ----
__global__ __launch_bounds__(256) void fg_adam_kernel(FgCtx ctx, float* p, const float* g_, float* m, float* v, long long n,
                                                      const float* __restrict__ lr_, const float* __restrict__ wd_,
                                                      const float* __restrict__ clip_, float b1, float b2, float eps,
                                                      const int* __restrict__ step_dev) {
  const int gm = blockIdx.y;
  if (fg_rows(ctx, gm) == 0) return;
  const long long off = gm * n;
  p += off; g_ += off; m += off; v += off;
  const float lr = lr_[gm], wd = wd_[gm], clip = clip_[gm];
  const int step = step_dev[gm] + 1;
  const float bc1 = 1.f - powf(b1, (float)step);
  const float bc2s = sqrtf(1.f - powf(b2, (float)step));
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    float gi = g_[i];
    if (clip > 0.f) gi = fminf(fmaxf(gi, -clip), clip);
    gi = fmaf(wd, p[i], gi);
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] - (lr / bc1) * (mi / (sqrtf(vi) / bc2s + eps));
  }
}

// ---- end of step: active models' step counters (train) and the step cursor advance.  One workgroup. ----
__global__ __launch_bounds__(256) void fg_finish_kernel(FgCtx c, int* step, int train, int* cursor) {
  for (int g = threadIdx.x; g < c.G; g += blockDim.x)
    if (train && fg_rows(c, g) > 0) step[g] += 1;
  __syncthreads();
  if (threadIdx.x == 0 && cursor) *cursor += 1;
}

__global__ __launch_bounds__(256) void fg_mask_kernel(uint64_t seed, int step, int site, int rows, int cols, float p, uint8_t* keep) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= (long long)rows * cols) return;
  keep[i] = fg_keep(seed, step, site, (int)(i / cols), (int)(i % cols), p) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side: parameter layout (model.parameters() order) and workspace layout (per model, floats)
// ---------------------------------------------------------------------------------------------------------------------
enum { FG_NLIN = 15, FG_FA = 12, FG_O1 = 13, FG_O2 = 14 };   // 0-8: {audio,text,video} x linear_{1,2,3}; 9-11: attention_mlp

struct FgPar {
  long long w[FG_NLIN], b[FG_NLIN], P;
  int out[FG_NLIN], in[FG_NLIN];
};
static FgPar fg_params(int Da, int Dt, int Dv, int H, int C1, int C2) {
  FgPar r;
  const int ins[FG_NLIN] = {Da, H, H, Dt, H, H, Dv, H, H, 3 * H, H, H, H, H, H};
  const int outs[FG_NLIN] = {H, H, H, H, H, H, H, H, H, H, H, H, 3, C1, C2};
  long long o = 0;
  for (int l = 0; l < FG_NLIN; ++l) {
    r.in[l] = ins[l];
    r.out[l] = outs[l];
    r.w[l] = o;
    o += (long long)outs[l] * ins[l];
    r.b[l] = o;
    o += outs[l];
  }
  r.P = o;
  return r;
}

struct FgLay {
  long long xa, xt, xv, emo, val, h1, h2, mh, mhd, a1, a2, a3, att, feat, eo, vo, demo, dval, dfeat, dmhf, datt, dza3, dza2, dza1,
      tmp, dze3, dze2, dze1, stride;
};
static FgLay fg_layout(const mer_fusion_group& d) {
  FgLay L;
  long long o = 0;
  auto take = [&](long long n) { const long long r = o; o += (n + 63) / 64 * 64; return r; };
  const long long B = d.B, H = d.H;
  L.xa = take(B * d.Da); L.xt = take(B * d.Dt); L.xv = take(B * d.Dv); L.emo = take(B); L.val = take(B);
  L.h1 = take(3 * B * H); L.h2 = take(3 * B * H); L.mh = take(3 * B * H); L.mhd = take(3 * B * H);
  L.a1 = take(B * H); L.a2 = take(B * H); L.a3 = take(B * H); L.att = take(3 * B); L.feat = take(B * H);
  L.eo = take(B * d.C1); L.vo = take(B * d.C2); L.demo = take(B * d.C1); L.dval = take(B * d.C2);
  L.dfeat = take(B * H); L.dmhf = take(3 * B * H); L.datt = take(3 * B);
  L.dza3 = take(B * H); L.dza2 = take(B * H); L.dza1 = take(B * H); L.tmp = take(3 * B * H);
  L.dze3 = take(3 * B * H); L.dze2 = take(3 * B * H); L.dze1 = take(3 * B * H);
  L.stride = o;
  return L;
}

static FgGemm fg_prob(const float* a, long long lda, long long a_gs, const float* w, long long ldw, long long w_gs, float* c,
                      long long ldc, long long c_gs, int M, int N, int K, int rows) {
  FgGemm p;
  p.a = a; p.lda = lda; p.a_gs = a_gs;
  p.w = w; p.ldw = ldw; p.w_gs = w_gs;
  p.c = c; p.ldc = ldc; p.c_gs = c_gs;
  p.bias = nullptr; p.bias_gs = 0; p.gate = nullptr; p.ldg = 0; p.gate_gs = 0;
  p.M = M; p.N = N; p.K = K; p.rows = rows; p.act = MER_ACT_NONE; p.accumulate = 0; p.tiles_n = 0; p.tile0 = 0;
  return p;
}

template <bool TA, bool TW>
static void fg_gemm(const FgCtx& ctx, FgGemmList& L, hipStream_t st) {
  int tiles = 0;
  for (int i = 0; i < L.np; ++i) {
    FgGemm& p = L.p[i];
    p.tiles_n = (int)cdiv(p.N, 16);
    p.tile0 = tiles;
    tiles += p.tiles_n * (int)cdiv(p.rows == 1 ? ctx.B : p.M, 16);
  }
  fg_gemm_kernel<TA, TW><<<dim3(tiles, ctx.G), 64, 0, st>>>(ctx, L);
}

}  // namespace mer

using namespace mer;

extern "C" long long mer_fusion_group_param_count(int Da, int Dt, int Dv, int H, int C1, int C2) {
  if (Da <= 0 || Dt <= 0 || Dv <= 0 || H <= 0 || C1 <= 0 || C2 <= 0) return MER_EINVAL;
  return fg_params(Da, Dt, Dv, H, C1, C2).P;
}

static int fg_check_shape(const mer_fusion_group* d) {
  MER_REQUIRE(d, MER_EINVAL, "mer_fusion_group: null descriptor");
  MER_REQUIRE(d->G > 0 && d->B > 0 && d->B <= FG_MAXB && d->n_steps > 0, MER_ESHAPE,
              "mer_fusion_group: need G > 0, 0 < B <= %d, n_steps > 0 (G=%d B=%d n_steps=%d)", FG_MAXB, d->G, d->B, d->n_steps);
  MER_REQUIRE(d->Da > 0 && d->Dt > 0 && d->Dv > 0 && d->H > 0 && d->Da < 65536 && d->Dt < 65536 && d->Dv < 65536 && 3 * d->H < 65536,
              MER_ESHAPE, "mer_fusion_group: bad dims Da=%d Dt=%d Dv=%d H=%d", d->Da, d->Dt, d->Dv, d->H);
  MER_REQUIRE(d->C1 > 0 && d->C1 <= 64 && d->C2 == 1, MER_EUNSUPPORTED,
              "mer_fusion_group: only the emotion (C1 <= 64) + valence (C2 = 1) heads are built (C1=%d C2=%d)", d->C1, d->C2);
  return MER_OK;
}

extern "C" long long mer_fusion_group_workspace_bytes(const mer_fusion_group* d) {
  const int rc = fg_check_shape(d);
  if (rc != MER_OK) return rc;
  return (long long)d->G * fg_layout(*d).stride * (long long)sizeof(float);
}

extern "C" int mer_fusion_group_step(const mer_fusion_group* d, int train, mer_stream_t stream) {
  const int rc = fg_check_shape(d);
  if (rc != MER_OK) return rc;
  const FgPar Pr = fg_params(d->Da, d->Dt, d->Dv, d->H, d->C1, d->C2);
  const FgLay Ly = fg_layout(*d);
  MER_REQUIRE(d->P == Pr.P, MER_ESHAPE, "mer_fusion_group_step: P=%lld, the architecture has %lld parameters", d->P, Pr.P);
  MER_REQUIRE(d->params && d->feat_a && d->feat_t && d->feat_v && d->emo && d->val && d->index && d->count && d->workspace &&
                  d->step && d->n_rows > 0,
              MER_EINVAL, "mer_fusion_group_step: null pointer");
  MER_REQUIRE(d->workspace_bytes >= (long long)d->G * Ly.stride * (long long)sizeof(float), MER_ENOMEM,
              "mer_fusion_group_step: workspace of %lld bytes, %lld needed", d->workspace_bytes,
              (long long)d->G * Ly.stride * (long long)sizeof(float));
  MER_REQUIRE(!train || (d->grads && d->adam_m && d->adam_v && d->lr && d->weight_decay && d->grad_clip && d->dropout), MER_EINVAL,
              "mer_fusion_group_step: a train step needs grads, Adam moments and the per-model lr / weight_decay / grad_clip / dropout");
  hipStream_t st = (hipStream_t)stream;
  const FgCtx ctx{d->cursor, d->count, d->G, d->B, d->n_steps};
  const int G = d->G, B = d->B, H = d->H, C1 = d->C1, C2 = d->C2;
  const long long S = Ly.stride, P = d->P;
  float* ws = (float*)d->workspace;
  float* par = d->params;
  float* grd = d->grads;
  const int Ds[3] = {d->Da, d->Dt, d->Dv};
  const long long xin[3] = {Ly.xa, Ly.xt, Ly.xv};
  const long long BH = (long long)B * H;

  fg_gather_kernel<<<dim3(B, G), 256, 0, st>>>(ctx, d->feat_a, d->feat_t, d->feat_v, d->emo, d->val, d->n_rows, d->index, d->Da,
                                               d->Dt, d->Dv, ws, S, Ly.xa, Ly.xt, Ly.xv, Ly.emo, Ly.val, train, d->dropout, d->seed,
                                               d->step);
  // ---- forward ----
  for (int layer = 0; layer < 3; ++layer) {   // the three MLPEncoders, one launch per layer
    FgGemmList L;
    L.np = 3;
    for (int e = 0; e < 3; ++e) {
      const int l = e * 3 + layer;
      const float* a = layer == 0 ? ws + xin[e] : ws + (layer == 1 ? Ly.h1 : Ly.h2) + e * BH;
      const long long lda = layer == 0 ? Ds[e] : H;
      float* c = layer == 2 ? ws + Ly.mh + e * H : ws + (layer == 0 ? Ly.h1 : Ly.h2) + e * BH;
      FgGemm p = fg_prob(a, lda, S, par + Pr.w[l], Pr.in[l], P, c, layer == 2 ? 3 * H : H, S, B, H, Pr.in[l], 1);
      p.bias = par + Pr.b[l]; p.bias_gs = P; p.act = MER_ACT_RELU;
      L.p[e] = p;
    }
    fg_gemm<false, false>(ctx, L, st);
  }
  if (train)
    fg_dropout_kernel<<<dim3(B, G), 256, 0, st>>>(ctx, ws, S, Ly.mh, Ly.mhd, 3 * H, d->dropout, d->seed, d->step, 3);
  const long long x_att = train ? Ly.mhd : Ly.mh;
  const long long att_in[3] = {x_att, Ly.a1, Ly.a2}, att_out[3] = {Ly.a1, Ly.a2, Ly.a3};
  for (int layer = 0; layer < 3; ++layer) {   // attention_mlp
    const int l = 9 + layer;
    FgGemmList L;
    L.np = 1;
    L.p[0] = fg_prob(ws + att_in[layer], Pr.in[l], S, par + Pr.w[l], Pr.in[l], P, ws + att_out[layer], H, S, B, H, Pr.in[l], 1);
    L.p[0].bias = par + Pr.b[l]; L.p[0].bias_gs = P; L.p[0].act = MER_ACT_RELU;
    fg_gemm<false, false>(ctx, L, st);
  }
  {
    FgGemmList L;
    L.np = 1;
    L.p[0] = fg_prob(ws + Ly.a3, H, S, par + Pr.w[FG_FA], H, P, ws + Ly.att, 3, S, B, 3, H, 1);
    L.p[0].bias = par + Pr.b[FG_FA]; L.p[0].bias_gs = P;
    fg_gemm<false, false>(ctx, L, st);
  }
  fg_fuse_fwd_kernel<<<dim3(B, G), 256, 0, st>>>(ctx, ws, S, Ly.mh, Ly.att, Ly.feat, H);
  {
    FgGemmList L;
    L.np = 2;
    L.p[0] = fg_prob(ws + Ly.feat, H, S, par + Pr.w[FG_O1], H, P, ws + Ly.eo, C1, S, B, C1, H, 1);
    L.p[0].bias = par + Pr.b[FG_O1]; L.p[0].bias_gs = P;
    L.p[1] = fg_prob(ws + Ly.feat, H, S, par + Pr.w[FG_O2], H, P, ws + Ly.vo, C2, S, B, C2, H, 1);
    L.p[1].bias = par + Pr.b[FG_O2]; L.p[1].bias_gs = P;
    fg_gemm<false, false>(ctx, L, st);
  }
  fg_loss_kernel<<<G, 256, 0, st>>>(ctx, ws, S, Ly.eo, Ly.vo, Ly.emo, Ly.val, Ly.demo, Ly.dval, C1, train, d->out_loss, d->out_emo,
                                    d->out_val);
  if (train) {
    // ---- backward: dX chain (relu_bwd folded into the stores through `gate`) ----
    {
      FgGemmList L;
      L.np = 1;
      L.p[0] = fg_prob(ws + Ly.demo, C1, S, par + Pr.w[FG_O1], H, P, ws + Ly.dfeat, H, S, B, H, C1, 1);
      fg_gemm<false, true>(ctx, L, st);
      L.p[0] = fg_prob(ws + Ly.dval, C2, S, par + Pr.w[FG_O2], H, P, ws + Ly.dfeat, H, S, B, H, C2, 1);
      L.p[0].accumulate = 1;   // dfeat = dX(fc_out_1) + dX(fc_out_2), autograd's two-term sum
      fg_gemm<false, true>(ctx, L, st);
    }
    fg_fuse_bwd_kernel<<<dim3(3 * B, G), 64, 0, st>>>(ctx, ws, S, Ly.dfeat, Ly.mh, Ly.att, Ly.dmhf, Ly.datt, H);
    {
      // fc_att, attention_mlp linear_3, linear_2: dX gated by the previous layer's ReLU output
      const int ls[3] = {FG_FA, 11, 10};
      const long long dz_in[3] = {Ly.datt, Ly.dza3, Ly.dza2}, dz_out[3] = {Ly.dza3, Ly.dza2, Ly.dza1}, gate[3] = {Ly.a3, Ly.a2, Ly.a1};
      for (int i = 0; i < 3; ++i) {
        const int l = ls[i];
        FgGemmList L;
        L.np = 1;
        L.p[0] = fg_prob(ws + dz_in[i], Pr.out[l], S, par + Pr.w[l], Pr.in[l], P, ws + dz_out[i], H, S, B, H, Pr.out[l], 1);
        L.p[0].gate = ws + gate[i]; L.p[0].ldg = H; L.p[0].gate_gs = S;
        fg_gemm<false, true>(ctx, L, st);
      }
      FgGemmList L;   // attention_mlp linear_1: dX w.r.t. its (dropped) input
      L.np = 1;
      L.p[0] = fg_prob(ws + Ly.dza1, H, S, par + Pr.w[9], 3 * H, P, ws + Ly.tmp, 3 * H, S, B, 3 * H, H, 1);
      fg_gemm<false, true>(ctx, L, st);
    }
    fg_mh_bwd_kernel<<<dim3(B, G), 256, 0, st>>>(ctx, ws, S, Ly.mh, Ly.dmhf, Ly.tmp, Ly.dze3, 3 * H, d->dropout, d->seed, d->step, 3);
    for (int layer = 2; layer >= 1; --layer) {   // encoders' linear_3, linear_2 dX
      FgGemmList L;
      L.np = 3;
      for (int e = 0; e < 3; ++e) {
        const int l = e * 3 + layer;
        const float* a = layer == 2 ? ws + Ly.dze3 + e * H : ws + Ly.dze2 + e * BH;
        const long long lda = layer == 2 ? 3 * H : H;
        float* c = ws + (layer == 2 ? Ly.dze2 : Ly.dze1) + e * BH;
        L.p[e] = fg_prob(a, lda, S, par + Pr.w[l], H, P, c, H, S, B, H, H, 1);
        L.p[e].gate = ws + (layer == 2 ? Ly.h2 : Ly.h1) + e * BH; L.p[e].ldg = H; L.p[e].gate_gs = S;
      }
      fg_gemm<false, true>(ctx, L, st);
    }
    // ---- weight gradients (dz^T x) and bias gradients (colsum dz) of all 15 linears: one launch each ----
    const float* dz[FG_NLIN];
    long long ldz[FG_NLIN];
    const float* xs[FG_NLIN];
    long long ldx[FG_NLIN];
    for (int e = 0; e < 3; ++e) {
      dz[e * 3 + 0] = ws + Ly.dze1 + e * BH; ldz[e * 3 + 0] = H; xs[e * 3 + 0] = ws + xin[e]; ldx[e * 3 + 0] = Ds[e];
      dz[e * 3 + 1] = ws + Ly.dze2 + e * BH; ldz[e * 3 + 1] = H; xs[e * 3 + 1] = ws + Ly.h1 + e * BH; ldx[e * 3 + 1] = H;
      dz[e * 3 + 2] = ws + Ly.dze3 + e * H; ldz[e * 3 + 2] = 3 * H; xs[e * 3 + 2] = ws + Ly.h2 + e * BH; ldx[e * 3 + 2] = H;
    }
    dz[9] = ws + Ly.dza1; ldz[9] = H; xs[9] = ws + x_att; ldx[9] = 3 * H;
    dz[10] = ws + Ly.dza2; ldz[10] = H; xs[10] = ws + Ly.a1; ldx[10] = H;
    dz[11] = ws + Ly.dza3; ldz[11] = H; xs[11] = ws + Ly.a2; ldx[11] = H;
    dz[FG_FA] = ws + Ly.datt; ldz[FG_FA] = 3; xs[FG_FA] = ws + Ly.a3; ldx[FG_FA] = H;
    dz[FG_O1] = ws + Ly.demo; ldz[FG_O1] = C1; xs[FG_O1] = ws + Ly.feat; ldx[FG_O1] = H;
    dz[FG_O2] = ws + Ly.dval; ldz[FG_O2] = C2; xs[FG_O2] = ws + Ly.feat; ldx[FG_O2] = H;
    {
      FgGemmList L;
      L.np = FG_NLIN;
      for (int l = 0; l < FG_NLIN; ++l)
        L.p[l] = fg_prob(dz[l], ldz[l], S, xs[l], ldx[l], S, grd + Pr.w[l], Pr.in[l], P, Pr.out[l], Pr.in[l], B, 2);
      fg_gemm<true, true>(ctx, L, st);
    }
    {
      FgSumList L;
      L.np = FG_NLIN;
      int blks = 0;
      for (int l = 0; l < FG_NLIN; ++l) {
        FgSum& s = L.p[l];
        s.x = dz[l]; s.ldx = ldz[l]; s.x_gs = S; s.out = grd + Pr.b[l]; s.out_gs = P; s.N = Pr.out[l]; s.blk0 = blks;
        blks += (int)cdiv(s.N, 64);
      }
      fg_colsum_kernel<<<dim3(blks, G), 64, 0, st>>>(ctx, L);
    }
    long long nb = cdiv(P, 256);
    nb = nb < 1 ? 1 : (nb > 1024 ? 1024 : nb);
    fg_adam_kernel<<<dim3((unsigned)nb, G), 256, 0, st>>>(ctx, par, grd, d->adam_m, d->adam_v, P, d->lr, d->weight_decay, d->grad_clip,
                                                          d->beta1, d->beta2, d->eps, d->step);
  }
  fg_finish_kernel<<<1, 256, 0, st>>>(ctx, d->step, train, d->cursor);
  return check_launch("fusion_group_step");
}

extern "C" int mer_fusion_group_dropout_mask(uint64_t seed, int step, int site, int rows, int cols, float p, uint8_t* keep,
                                             mer_stream_t stream) {
  MER_REQUIRE(keep && rows > 0 && cols > 0 && rows <= 16384 && cols < 65536 && site >= 0 && site < 4, MER_EINVAL,
              "mer_fusion_group_dropout_mask: bad args (rows=%d cols=%d site=%d)", rows, cols, site);
  fg_mask_kernel<<<(unsigned)cdiv((long long)rows * cols, 256), 256, 0, (hipStream_t)stream>>>(seed, step, site, rows, cols, p, keep);
  return check_launch("fusion_group_dropout_mask");
}
