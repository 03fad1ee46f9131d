// fusion_topn_group.hip — the group engine: one training (or evaluation) step for a GROUP of G independent fusion models of
// one architecture, the 5 folds of a cross-validation run times N hyper-parameter trials.  Two C ABIs run on it:
//   mer_fusion_topn_group_*  Attention_TOPN (MER2024/toolkit/models/attention_topn.py: M feature streams, 1 <= M <= 18,
//                            feat_type 'utt', an emotion head of C1 classes and a valence head of C2 in {0, 1} outputs), the
//                            MER2024 / MER2025 / MER2026 multi-feature recipe;
//   mer_fusion_group_*       Attention (MERBench/toolkit/models/attention.py:36-57 with feat_type 'utt', both heads;
//                            main-release.py:31-66), MER2023: the same model with M = 3 (audio, text, video) and C2 = 1.  Its
//                            entry points (end of this file) map their descriptor onto the engine's.
// The model index is a grid axis of every launch and the M streams are entries of grouped problem lists, so the number of
// launches of a step depends on neither G nor M (25 for a train step with C2 = 0, 26 with C2 = 1, 12 for an eval step);
// every stage is an ordinary launch on one stream (no inter-workgroup communication), and a step allocates nothing and never
// synchronises (graph-capturable).
//
// Arithmetic contract: each stage is the per-element arithmetic of the single-model kernels (gemm32.hip's MFMA k grouping and
// epilogue, fusion.hip's fuse forward — an fmaf chain over the streams in stream order — and backward, CE / MSE rows and their
// in-order means, Adam), with the row count of a model (n_g <= B) taking the place of the minibatch size.  So model g's losses,
// outputs, gradients and parameters are bitwise those of a group holding g alone, and for M = 3, C2 = 1, dropout 0 bitwise
// those of FusionGraphTrainer on the same minibatches, through either ABI.  With C2 = 0 the loss is CE alone and there is no
// valence output or gradient.  A model with n_g = 0 is idle: its parameters, gradients, Adam moments and step counter are not
// touched.
//
// Problem lists travel by value as kernel arguments.  A list holds up to 3 * 18 + 6 = 60 problems (the weight gradients of
// every Linear of an 18-stream model), so a problem is a compact 64-byte record of offsets into the launch's base pointers
// (workspace, parameters or gradients — one base per operand and launch); with the context and the bases the argument block
// is 3960 bytes, under HIP's 4 KB limit (static_assert below).
//
// Dropout keep mask (stateless, counter-based; site i < M = input of encoder i, site M = input of attention_mlp):
//   ctr  = (uint64(uint32(step)) << 32) | (site << shift) | (row << 16) | col
//   z    = seed + (ctr + 1) * 0x9E3779B97F4A7C15                                 (mod 2^64)
//   z    = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31   (splitmix64)
//   u    = float(z >> 40) * 2^-24;   keep = u >= p;   out = keep ? x * (1.0f / (1.0f - p)) : 0      (fp32)
// step is the model's optimiser step counter before the step, row the row within the minibatch.  The two ABIs differ in the
// field widths of the counter and in nothing else, and each layout is a documented contract with an exact test:
//   mer_fusion_topn_group_*  shift = 27   (site < 32, row < 2^11, col < 2^16; 19 sites do not fit a 2-bit field)
//   mer_fusion_group_*       shift = 30   (site 0/1/2 = audio/text/video encoder input, 3 = attention_mlp input; row < 2^14)
// The shift travels in TgCtx (TgCtx::site_shift) and is an argument of tg_keep and tg_mask_kernel.
#include "common.h"

namespace mer {

#define TG_MAXS MER_TOPN_MAX_STREAMS
#define TG_MAXP (3 * TG_MAXS + 6)
#define TG_MAXB 2048

struct TgCtx {
  const int* cursor;
  const int* count;
  int G, B, S;
  int site_shift;   // dropout counter layout: 27 (mer_fusion_topn_group_*) or 30 (mer_fusion_group_*)
};
static_assert(sizeof(TgCtx) == 32, "site_shift lives in TgCtx's tail padding");

// rows of model g in the current step (0 = idle; also 0 once the cursor ran past the step table)
__device__ __forceinline__ int tg_rows(const TgCtx& c, int g) {
  const int s = c.cursor ? *c.cursor : 0;
  if (s < 0 || s >= c.S) return 0;
  const int n = c.count[(long long)s * c.G + g];
  return n < 0 ? 0 : (n > c.B ? c.B : n);
}
__device__ __forceinline__ long long tg_slot(const TgCtx& c, int g) {
  return (long long)(c.cursor ? *c.cursor : 0) * c.G + g;
}

__host__ __device__ __forceinline__ uint64_t tg_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ __forceinline__ bool tg_keep(uint64_t seed, int step, int site, int row, int col, float p, int shift) {
  const uint64_t ctr = ((uint64_t)(uint32_t)step << 32) | ((uint64_t)site << shift) | ((uint64_t)row << 16) | (uint64_t)col;
  const uint64_t z = tg_mix(seed + (ctr + 1ull) * 0x9E3779B97F4A7C15ull);
  return (float)(z >> 40) * (1.0f / 16777216.0f) >= p;
}

// ---- row gather (+ inverted dropout of the M encoder inputs on train steps).  grid (B, G) ----
struct TgTabs {
  const float* feat[TG_MAXS];
  long long o_x[TG_MAXS];
  int D[TG_MAXS];
  int M;
};
__global__ __launch_bounds__(256) void tg_gather_kernel(TgCtx c, const TgTabs T, const int* __restrict__ emo_tab,
                                                        const float* __restrict__ val_tab, long long n_rows, const int* __restrict__ index,
                                                        float* ws, long long ws_gs, long long o_emo, long long o_val, int train,
                                                        const float* __restrict__ drop, const uint64_t* __restrict__ seed,
                                                        const int* __restrict__ step) {
  const int r = blockIdx.x, g = blockIdx.y;
  if (r >= tg_rows(c, g)) return;
  const long long src = index[tg_slot(c, g) * c.B + r];
  const bool ok = src >= 0 && src < n_rows;
  float* w = ws + g * ws_gs;
  const float p = train ? drop[g] : 0.f;
  const float scale = 1.0f / (1.0f - p);
  const uint64_t sd = seed ? seed[g] : 0ull;
  const int st = train ? step[g] : 0;
  for (int e = 0; e < T.M; ++e) {
    const int D = T.D[e];
    const float* tab = T.feat[e];
    float* dst = w + T.o_x[e] + (long long)r * D;
    for (int j = threadIdx.x; j < D; j += blockDim.x) {
      const float x = ok ? tab[src * D + j] : 0.f;
      dst[j] = p > 0.f ? (tg_keep(sd, st, e, r, j, p, c.site_shift) ? x * scale : 0.f) : x;
    }
  }
  if (threadIdx.x == 0) {
    reinterpret_cast<int*>(w + o_emo)[r] = ok ? emo_tab[src] : 0;
    if (val_tab) w[o_val + r] = ok ? val_tab[src] : 0.f;
  }
}

// ---- grouped exact-fp32 GEMM: gemm32.hip's tile (v_mfma_f32_16x16x4f32, same k grouping and epilogue) over a list of
// problems; grid (sum of the problems' tiles, G).  rows == 1: M is the model's row count (forward, dX); rows == 2: K is (dW).
// gate >= 0 folds relu_bwd into the store: v = gate[row, col] > 0 ? v : 0.  bias != 0: the N floats that follow the [N, K]
// weight (a Linear's bias in model.parameters() order). ----
struct TgGemm {
  long long a, w, c, gate;   // float offsets from TgBase's pointers (per model: + g * the base's group stride)
  int lda, ldw, ldc, M, N, K, tile0, bias;
};
struct TgBase {
  const float* a; const float* w; float* c; const float* gate;
  long long a_gs, w_gs, c_gs, gate_gs;
  int rows, act, accumulate, ldg;
};
struct TgGemmList {
  TgGemm p[TG_MAXP];
  int np;
};
static_assert(sizeof(TgGemm) == 64, "TgGemm is a 64-byte record");
static_assert(sizeof(TgCtx) + sizeof(TgBase) + sizeof(TgGemmList) <= 4096, "kernel arguments must stay under 4 KB");

template <bool TA, bool TW>
__global__ __launch_bounds__(64) void tg_gemm_kernel(TgCtx ctx, const TgBase Bs, const TgGemmList L) {
  const int g = blockIdx.y;
  const int ng = tg_rows(ctx, g);
  if (ng == 0) return;
  int pi = 0;
  for (int i = 1; i < L.np; ++i)
    if ((int)blockIdx.x >= L.p[i].tile0) pi = i;
  const TgGemm& P = L.p[pi];
  const int t = (int)blockIdx.x - P.tile0;
  const int tiles_n = (P.N + 15) / 16;
  const int tn = t % tiles_n, tm = t / tiles_n;
  const int M = Bs.rows == 1 ? ng : P.M, N = P.N, K = Bs.rows == 2 ? ng : P.K;
  if (tm * 16 >= M) return;
  const float* __restrict__ a = Bs.a + g * Bs.a_gs + P.a;
  const float* __restrict__ w = Bs.w + g * Bs.w_gs + P.w;
  const float* bias = P.bias ? w + (long long)P.N * P.K : nullptr;
  const float* gate = P.gate >= 0 ? Bs.gate + g * Bs.gate_gs + P.gate : nullptr;
  float* c = Bs.c + g * Bs.c_gs + P.c;
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
      float v = act_apply(acc[r] + bv, Bs.act);
      if (gate) v = gate[(long long)row * Bs.ldg + col] > 0.f ? v : 0.f;
      float* dst = c + (long long)row * ldc + col;
      *dst = Bs.accumulate ? *dst + v : v;
    }
  }
}

// ---- attention_mlp input dropout (site M).  grid (B, G) ----
__global__ __launch_bounds__(256) void tg_dropout_kernel(TgCtx c, float* ws, long long ws_gs, long long o_x, long long o_y, int W,
                                                         const float* __restrict__ drop, const uint64_t* __restrict__ seed,
                                                         const int* __restrict__ step, int site) {
  const int r = blockIdx.x, g = blockIdx.y;
  if (r >= tg_rows(c, g)) return;
  const float* x = ws + g * ws_gs + o_x + (long long)r * W;
  float* y = ws + g * ws_gs + o_y + (long long)r * W;
  const float p = drop[g];
  const float scale = 1.0f / (1.0f - p);
  const uint64_t sd = seed ? seed[g] : 0ull;
  const int st = step[g];
  for (int j = threadIdx.x; j < W; j += blockDim.x)
    y[j] = p > 0.f ? (tg_keep(sd, st, site, r, j, p, c.site_shift) ? x[j] * scale : 0.f) : x[j];
}

// ---- fuse_fwd: feat[b,j] = sum_e mh[b, e*H + j] * att[b,e] (fmaf chain, e in stream order).  grid (B, G) ----
__global__ __launch_bounds__(256) void tg_fuse_fwd_kernel(TgCtx c, float* ws, long long ws_gs, long long o_h, long long o_att,
                                                          long long o_out, int H, int E) {
  const int b = blockIdx.x, g = blockIdx.y;
  if (b >= tg_rows(c, g)) return;
  const float* h = ws + g * ws_gs + o_h;
  const float* att = ws + g * ws_gs + o_att;
  float* out = ws + g * ws_gs + o_out;
  for (int j = threadIdx.x; j < H; j += blockDim.x) {
    float s = 0.f;
    for (int e = 0; e < E; ++e) s = fmaf(h[(long long)b * E * H + e * H + j], att[b * E + e], s);
    out[(long long)b * H + j] = s;
  }
}

// ---- fuse_bwd: dh[b,e*H+j] = dout[b,j]*att[b,e]; datt[b,e] = wave_sum of dout*h (fusion.hip's lane split).  grid (E*B, G) ----
__global__ __launch_bounds__(64) void tg_fuse_bwd_kernel(TgCtx c, float* ws, long long ws_gs, long long o_dout, long long o_h,
                                                         long long o_att, long long o_dh, long long o_datt, int H, int E) {
  const int b = blockIdx.x / E, e = blockIdx.x % E, g = blockIdx.y, lane = threadIdx.x;
  if (b >= tg_rows(c, g)) return;
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

// ---- CE (+ MSE when C2 = 1) rows, their means in row order, the step loss, the outputs into the epoch buffers and (train)
// the loss gradients.  One workgroup of 4 waves per model; CE rows one wave each (fusion.hip's ce_rows lane split). ----
__global__ __launch_bounds__(256) void tg_loss_kernel(TgCtx c, float* ws, long long ws_gs, long long o_eo, long long o_vo,
                                                      long long o_emo, long long o_val, long long o_demo, long long o_dval, int C1,
                                                      int C2, int train, float* out_loss, float* out_emo, float* out_val) {
  __shared__ float ce_row[TG_MAXB];
  __shared__ float mse_row[TG_MAXB];
  const int g = blockIdx.x;
  const int n = tg_rows(c, g);
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
  if (C2) {
    for (int b = threadIdx.x; b < n; b += blockDim.x) {
      const float d = vo[b] - vl[b];
      mse_row[b] = d * d;
      if (train) base[o_dval + b] = 2.f * (vo[b] - vl[b]) / (float)n;
    }
  }
  const long long slot = tg_slot(c, g);
  if (out_emo)
    for (int i = threadIdx.x; i < n * C1; i += blockDim.x) out_emo[slot * c.B * C1 + i] = lg[i];
  if (C2 && out_val)
    for (int b = threadIdx.x; b < n; b += blockDim.x) out_val[slot * c.B + b] = vo[b];
  __syncthreads();
  if (threadIdx.x == 0 && out_loss) {
    float s = 0.f;
    for (int b = 0; b < n; ++b) s += ce_row[b];
    const float ce = s / (float)n;
    if (C2) {
      s = 0.f;
      for (int b = 0; b < n; ++b) s += mse_row[b];
      const float mse = s / (float)n;
      out_loss[slot] = ce + mse;
    } else {
      out_loss[slot] = ce;
    }
  }
}

// ---- encoders' L3 gradient: dz[b,c] = mh[b,c] > 0 ? dh_fuse[b,c] + dropout_bwd(dx_att1)[b,c] : 0.  grid (B, G) ----
__global__ __launch_bounds__(256) void tg_mh_bwd_kernel(TgCtx c, float* ws, long long ws_gs, long long o_mh, long long o_dhf,
                                                        long long o_dxa, long long o_dz, int W, const float* __restrict__ drop,
                                                        const uint64_t* __restrict__ seed, const int* __restrict__ step, int site) {
  const int r = blockIdx.x, g = blockIdx.y;
  if (r >= tg_rows(c, g)) return;
  float* base = ws + g * ws_gs;
  const long long o = (long long)r * W;
  const float p = drop[g];
  const float scale = 1.0f / (1.0f - p);
  const uint64_t sd = seed ? seed[g] : 0ull;
  const int st = step[g];
  for (int j = threadIdx.x; j < W; j += blockDim.x) {
    const float dx = base[o_dxa + o + j];
    const float dd = p > 0.f ? (tg_keep(sd, st, site, r, j, p, c.site_shift) ? dx * scale : 0.f) : dx;
    const float dy = base[o_dhf + o + j] + dd;
    base[o_dz + o + j] = base[o_mh + o + j] > 0.f ? dy : 0.f;
  }
}

// ---- bias gradients: out[n] = sum over the model's rows of x[m, n], rows in order.  grid (sum of 64-column blocks, G) ----
struct TgSum {
  long long x, out;   // float offsets into the workspace / the gradient buffer
  int ldx, N, blk0, pad;
};
struct TgSumList {
  TgSum p[TG_MAXP];
  int np;
};
__global__ __launch_bounds__(64) void tg_colsum_kernel(TgCtx ctx, const float* __restrict__ ws, long long ws_gs, float* grads,
                                                       long long grads_gs, const TgSumList L) {
  const int g = blockIdx.y;
  const int M = tg_rows(ctx, g);
  if (M == 0) return;
  int pi = 0;
  for (int i = 1; i < L.np; ++i)
    if ((int)blockIdx.x >= L.p[i].blk0) pi = i;
  const TgSum& P = L.p[pi];
  const int n = ((int)blockIdx.x - P.blk0) * 64 + threadIdx.x;
  if (n >= P.N) return;
  const float* x = ws + g * ws_gs + P.x;
  float s = 0.f;
  for (int m = 0; m < M; ++m) s += x[(long long)m * P.ldx + n];
  grads[g * grads_gs + P.out + n] = s;
}

// ---- Adam (fusion.hip adam_dev_kernel's arithmetic) with per-model lr / weight decay / clip.  grid (blocks, G) ----
__global__ __launch_bounds__(256) void tg_adam_kernel(TgCtx ctx, float* p, const float* g_, float* m, float* v, long long n,
                                                      const float* __restrict__ lr_, const float* __restrict__ wd_,
                                                      const float* __restrict__ clip_, float b1, float b2, float eps,
                                                      const int* __restrict__ step_dev) {
  const int gm = blockIdx.y;
  if (tg_rows(ctx, gm) == 0) return;
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
__global__ __launch_bounds__(256) void tg_finish_kernel(TgCtx c, int* step, int train, int* cursor) {
  for (int g = threadIdx.x; g < c.G; g += blockDim.x)
    if (train && tg_rows(c, g) > 0) step[g] += 1;
  __syncthreads();
  if (threadIdx.x == 0 && cursor) *cursor += 1;
}

__global__ __launch_bounds__(256) void tg_mask_kernel(uint64_t seed, int step, int site, int rows, int cols, float p, uint8_t* keep,
                                                      int shift) {
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if (i >= (long long)rows * cols) return;
  keep[i] = tg_keep(seed, step, site, (int)(i / cols), (int)(i % cols), p, shift) ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// host side: parameter layout (model.parameters() order) and workspace layout (per model, floats)
// ---------------------------------------------------------------------------------------------------------------------
// linears: 3e + {0,1,2} = encoder e's linear_{1,2,3}; A0 + {0,1,2} = attention_mlp; FA = fc_att; O1, O2 = fc_out_1, fc_out_2
struct TgPar {
  long long w[TG_MAXP], b[TG_MAXP], P;
  int out[TG_MAXP], in[TG_MAXP];
  int nlin, A0, FA, O1, O2;
};
static TgPar tg_params(int M, const int* D, int H, int C1, int C2) {
  TgPar r;
  r.A0 = 3 * M; r.FA = 3 * M + 3; r.O1 = 3 * M + 4; r.O2 = 3 * M + 5; r.nlin = 3 * M + 6;
  for (int e = 0; e < M; ++e)
    for (int l = 0; l < 3; ++l) {
      r.in[3 * e + l] = l == 0 ? D[e] : H;
      r.out[3 * e + l] = H;
    }
  for (int l = 0; l < 3; ++l) {
    r.in[r.A0 + l] = l == 0 ? M * H : H;
    r.out[r.A0 + l] = H;
  }
  r.in[r.FA] = H; r.out[r.FA] = M;
  r.in[r.O1] = H; r.out[r.O1] = C1;
  r.in[r.O2] = H; r.out[r.O2] = C2;
  long long o = 0;
  for (int l = 0; l < r.nlin; ++l) {
    r.w[l] = o;
    o += (long long)r.out[l] * r.in[l];
    r.b[l] = o;
    o += r.out[l];
  }
  r.P = o;
  return r;
}

struct TgLay {
  long long x[TG_MAXS], emo, val, h1, h2, mh, mhd, a1, a2, a3, att, feat, eo, vo, demo, dval, dfeat, dmhf, datt, dza3, dza2, dza1,
      tmp, dze3, dze2, dze1, stride;
};
static TgLay tg_layout(const mer_fusion_topn_group& d) {
  TgLay L;
  long long o = 0;
  auto take = [&](long long n) { const long long r = o; o += (n + 63) / 64 * 64; return r; };
  const long long B = d.B, H = d.H, M = d.M;
  for (int e = 0; e < TG_MAXS; ++e) L.x[e] = e < d.M ? take(B * d.D[e]) : 0;
  L.emo = take(B); L.val = take(B);
  L.h1 = take(M * B * H); L.h2 = take(M * B * H); L.mh = take(M * B * H); L.mhd = take(M * B * H);
  L.a1 = take(B * H); L.a2 = take(B * H); L.a3 = take(B * H); L.att = take(M * B); L.feat = take(B * H);
  L.eo = take(B * d.C1); L.vo = take(B * d.C2); L.demo = take(B * d.C1); L.dval = take(B * d.C2);
  L.dfeat = take(B * H); L.dmhf = take(M * B * H); L.datt = take(M * B);
  L.dza3 = take(B * H); L.dza2 = take(B * H); L.dza1 = take(B * H); L.tmp = take(M * B * H);
  L.dze3 = take(M * B * H); L.dze2 = take(M * B * H); L.dze1 = take(M * B * H);
  L.stride = o;
  return L;
}

static TgGemm tg_prob(long long a, long long lda, long long w, long long ldw, long long c, long long ldc, int M, int N, int K) {
  TgGemm p;
  p.a = a; p.lda = (int)lda;
  p.w = w; p.ldw = (int)ldw;
  p.c = c; p.ldc = (int)ldc;
  p.gate = -1; p.bias = 0;
  p.M = M; p.N = N; p.K = K; p.tile0 = 0;
  return p;
}

// operand bases of the three launch kinds: forward / dX read the workspace and the parameters and write the workspace;
// dW reads the workspace twice and writes the gradient buffer
static TgBase tg_base_fwd(float* ws, long long S, const float* par, long long P, int act) {
  TgBase b;
  b.a = ws; b.a_gs = S; b.w = par; b.w_gs = P; b.c = ws; b.c_gs = S; b.gate = ws; b.gate_gs = S;
  b.rows = 1; b.act = act; b.accumulate = 0; b.ldg = 0;
  return b;
}

template <bool TA, bool TW>
static void tg_gemm(const TgCtx& ctx, const TgBase& Bs, TgGemmList& L, hipStream_t st) {
  int tiles = 0;
  for (int i = 0; i < L.np; ++i) {
    TgGemm& p = L.p[i];
    p.tile0 = tiles;
    tiles += (int)cdiv(p.N, 16) * (int)cdiv(Bs.rows == 1 ? ctx.B : p.M, 16);
  }
  tg_gemm_kernel<TA, TW><<<dim3(tiles, ctx.G), 64, 0, st>>>(ctx, Bs, L);
}

}  // namespace mer

using namespace mer;

static int tg_check_dims(const char* fn, int M, const int* D, int H, int C1, int C2) {
  MER_REQUIRE(M >= 1 && M <= TG_MAXS, MER_ESHAPE, "%s: M = %d streams, 1..%d are built", fn, M, TG_MAXS);
  MER_REQUIRE(D, MER_EINVAL, "%s: null stream widths", fn);
  for (int e = 0; e < M; ++e)
    MER_REQUIRE(D[e] > 0 && D[e] < 65536, MER_ESHAPE, "%s: stream %d has width %d, need 0 < D < 65536", fn, e, D[e]);
  MER_REQUIRE(H > 0 && (long long)M * H < 65536, MER_ESHAPE, "%s: need H > 0 and M * H < 65536 (M=%d H=%d)", fn, M, H);
  MER_REQUIRE(C1 >= 1 && C1 <= 64, MER_ESHAPE, "%s: C1 = %d emotion classes, 1..64 are built", fn, C1);
  MER_REQUIRE(C2 == 0 || C2 == 1, MER_ESHAPE, "%s: C2 = %d valence outputs, 0 or 1 are built", fn, C2);
  return MER_OK;
}

extern "C" long long mer_fusion_topn_group_param_count(int M, const int* D, int H, int C1, int C2) {
  const int rc = tg_check_dims("mer_fusion_topn_group_param_count", M, D, H, C1, C2);
  if (rc != MER_OK) return rc;
  return tg_params(M, D, H, C1, C2).P;
}

static int tg_check_shape(const char* fn, const mer_fusion_topn_group* d) {
  MER_REQUIRE(d, MER_EINVAL, "%s: null descriptor", fn);
  const int rc = tg_check_dims(fn, d->M, d->D, d->H, d->C1, d->C2);
  if (rc != MER_OK) return rc;
  MER_REQUIRE(d->G > 0 && d->B > 0 && d->B <= TG_MAXB && d->n_steps > 0, MER_ESHAPE,
              "%s: need G > 0, 0 < B <= %d, n_steps > 0 (G=%d B=%d n_steps=%d)", fn, TG_MAXB, d->G, d->B, d->n_steps);
  return MER_OK;
}

extern "C" long long mer_fusion_topn_group_workspace_bytes(const mer_fusion_topn_group* d) {
  const int rc = tg_check_shape("mer_fusion_topn_group_workspace_bytes", d);
  if (rc != MER_OK) return rc;
  return (long long)d->G * tg_layout(*d).stride * (long long)sizeof(float);
}

// One step of the engine for either ABI: `fn` names the entry point in every error, `site_shift` is its dropout counter layout.
static int tg_step(const char* fn, const mer_fusion_topn_group* d, int site_shift, int train, mer_stream_t stream) {
  const int rc = tg_check_shape(fn, d);
  if (rc != MER_OK) return rc;
  const int G = d->G, B = d->B, H = d->H, C1 = d->C1, C2 = d->C2, M = d->M;
  const TgPar Pr = tg_params(M, d->D, H, C1, C2);
  const TgLay Ly = tg_layout(*d);
  MER_REQUIRE(d->P == Pr.P, MER_ESHAPE, "%s: P=%lld, the architecture has %lld parameters", fn, d->P, Pr.P);
  MER_REQUIRE(d->params && d->emo && d->index && d->count && d->workspace && d->step && d->n_rows > 0 && (C2 == 0 || d->val),
              MER_EINVAL, "%s: null pointer", fn);
  for (int e = 0; e < M; ++e) MER_REQUIRE(d->feat[e], MER_EINVAL, "%s: null feature table %d", fn, e);
  MER_REQUIRE(d->workspace_bytes >= (long long)G * Ly.stride * (long long)sizeof(float), MER_ENOMEM,
              "%s: workspace of %lld bytes, %lld needed", fn, d->workspace_bytes,
              (long long)G * Ly.stride * (long long)sizeof(float));
  MER_REQUIRE(!train || (d->grads && d->adam_m && d->adam_v && d->lr && d->weight_decay && d->grad_clip && d->dropout), MER_EINVAL,
              "%s: a train step needs grads, Adam moments and the per-model lr / weight_decay / grad_clip / dropout", fn);
  hipStream_t st = (hipStream_t)stream;
  const TgCtx ctx{d->cursor, d->count, G, B, d->n_steps, site_shift};
  const long long S = Ly.stride, P = d->P;
  float* ws = (float*)d->workspace;
  float* par = d->params;
  float* grd = d->grads;
  const long long BH = (long long)B * H;
  const int MH = M * H;

  {
    TgTabs T;
    T.M = M;
    for (int e = 0; e < TG_MAXS; ++e) {
      T.feat[e] = e < M ? d->feat[e] : nullptr;
      T.o_x[e] = Ly.x[e];
      T.D[e] = e < M ? d->D[e] : 0;
    }
    tg_gather_kernel<<<dim3(B, G), 256, 0, st>>>(ctx, T, d->emo, C2 ? d->val : nullptr, d->n_rows, d->index, ws, S, Ly.emo, Ly.val,
                                                 train, d->dropout, d->seed, d->step);
  }
  // ---- forward ----
  const TgBase relu = tg_base_fwd(ws, S, par, P, MER_ACT_RELU), plain = tg_base_fwd(ws, S, par, P, MER_ACT_NONE);
  for (int layer = 0; layer < 3; ++layer) {   // the M MLPEncoders, one launch per layer
    TgGemmList L;
    L.np = M;
    for (int e = 0; e < M; ++e) {
      const int l = e * 3 + layer;
      const long long a = layer == 0 ? Ly.x[e] : (layer == 1 ? Ly.h1 : Ly.h2) + e * BH;
      const long long lda = layer == 0 ? d->D[e] : H;
      const long long c = layer == 2 ? Ly.mh + e * H : (layer == 0 ? Ly.h1 : Ly.h2) + e * BH;
      L.p[e] = tg_prob(a, lda, Pr.w[l], Pr.in[l], c, layer == 2 ? MH : H, B, H, Pr.in[l]);
      L.p[e].bias = 1;
    }
    tg_gemm<false, false>(ctx, relu, L, st);
  }
  if (train)
    tg_dropout_kernel<<<dim3(B, G), 256, 0, st>>>(ctx, ws, S, Ly.mh, Ly.mhd, MH, d->dropout, d->seed, d->step, M);
  const long long x_att = train ? Ly.mhd : Ly.mh;
  const long long att_in[3] = {x_att, Ly.a1, Ly.a2}, att_out[3] = {Ly.a1, Ly.a2, Ly.a3};
  for (int layer = 0; layer < 3; ++layer) {   // attention_mlp
    const int l = Pr.A0 + layer;
    TgGemmList L;
    L.np = 1;
    L.p[0] = tg_prob(att_in[layer], Pr.in[l], Pr.w[l], Pr.in[l], att_out[layer], H, B, H, Pr.in[l]);
    L.p[0].bias = 1;
    tg_gemm<false, false>(ctx, relu, L, st);
  }
  {
    TgGemmList L;
    L.np = 1;
    L.p[0] = tg_prob(Ly.a3, H, Pr.w[Pr.FA], H, Ly.att, M, B, M, H);
    L.p[0].bias = 1;
    tg_gemm<false, false>(ctx, plain, L, st);
  }
  tg_fuse_fwd_kernel<<<dim3(B, G), 256, 0, st>>>(ctx, ws, S, Ly.mh, Ly.att, Ly.feat, H, M);
  {
    TgGemmList L;
    L.np = 1;
    L.p[0] = tg_prob(Ly.feat, H, Pr.w[Pr.O1], H, Ly.eo, C1, B, C1, H);
    L.p[0].bias = 1;
    if (C2) {
      L.np = 2;
      L.p[1] = tg_prob(Ly.feat, H, Pr.w[Pr.O2], H, Ly.vo, C2, B, C2, H);
      L.p[1].bias = 1;
    }
    tg_gemm<false, false>(ctx, plain, L, st);
  }
  tg_loss_kernel<<<G, 256, 0, st>>>(ctx, ws, S, Ly.eo, Ly.vo, Ly.emo, Ly.val, Ly.demo, Ly.dval, C1, C2, train, d->out_loss,
                                    d->out_emo, d->out_val);
  if (train) {
    // ---- backward: dX chain (relu_bwd folded into the stores through `gate`) ----
    TgBase dx = plain;
    dx.ldg = H;
    {
      TgGemmList L;
      L.np = 1;
      L.p[0] = tg_prob(Ly.demo, C1, Pr.w[Pr.O1], H, Ly.dfeat, H, B, H, C1);
      tg_gemm<false, true>(ctx, dx, L, st);
      if (C2) {
        L.p[0] = tg_prob(Ly.dval, C2, Pr.w[Pr.O2], H, Ly.dfeat, H, B, H, C2);
        TgBase acc = dx;
        acc.accumulate = 1;   // dfeat = dX(fc_out_1) + dX(fc_out_2), autograd's two-term sum
        tg_gemm<false, true>(ctx, acc, L, st);
      }
    }
    tg_fuse_bwd_kernel<<<dim3(M * B, G), 64, 0, st>>>(ctx, ws, S, Ly.dfeat, Ly.mh, Ly.att, Ly.dmhf, Ly.datt, H, M);
    {
      // fc_att, attention_mlp linear_3, linear_2: dX gated by the previous layer's ReLU output
      const int ls[3] = {Pr.FA, Pr.A0 + 2, Pr.A0 + 1};
      const long long dz_in[3] = {Ly.datt, Ly.dza3, Ly.dza2}, dz_out[3] = {Ly.dza3, Ly.dza2, Ly.dza1}, gate[3] = {Ly.a3, Ly.a2, Ly.a1};
      for (int i = 0; i < 3; ++i) {
        const int l = ls[i];
        TgGemmList L;
        L.np = 1;
        L.p[0] = tg_prob(dz_in[i], Pr.out[l], Pr.w[l], Pr.in[l], dz_out[i], H, B, H, Pr.out[l]);
        L.p[0].gate = gate[i];
        tg_gemm<false, true>(ctx, dx, L, st);
      }
      TgGemmList L;   // attention_mlp linear_1: dX w.r.t. its (dropped) input
      L.np = 1;
      L.p[0] = tg_prob(Ly.dza1, H, Pr.w[Pr.A0], MH, Ly.tmp, MH, B, MH, H);
      tg_gemm<false, true>(ctx, dx, L, st);
    }
    tg_mh_bwd_kernel<<<dim3(B, G), 256, 0, st>>>(ctx, ws, S, Ly.mh, Ly.dmhf, Ly.tmp, Ly.dze3, MH, d->dropout, d->seed, d->step, M);
    for (int layer = 2; layer >= 1; --layer) {   // encoders' linear_3, linear_2 dX
      TgGemmList L;
      L.np = M;
      for (int e = 0; e < M; ++e) {
        const int l = e * 3 + layer;
        const long long a = layer == 2 ? Ly.dze3 + e * H : Ly.dze2 + e * BH;
        const long long lda = layer == 2 ? MH : H;
        const long long c = (layer == 2 ? Ly.dze2 : Ly.dze1) + e * BH;
        L.p[e] = tg_prob(a, lda, Pr.w[l], H, c, H, B, H, H);
        L.p[e].gate = (layer == 2 ? Ly.h2 : Ly.h1) + e * BH;
      }
      tg_gemm<false, true>(ctx, dx, L, st);
    }
    // ---- weight gradients (dz^T x) and bias gradients (colsum dz) of all 3M + 6 linears: one launch each ----
    long long dz[TG_MAXP], xs[TG_MAXP];
    int ldz[TG_MAXP], ldx[TG_MAXP];
    for (int e = 0; e < M; ++e) {
      dz[e * 3 + 0] = Ly.dze1 + e * BH; ldz[e * 3 + 0] = H; xs[e * 3 + 0] = Ly.x[e]; ldx[e * 3 + 0] = d->D[e];
      dz[e * 3 + 1] = Ly.dze2 + e * BH; ldz[e * 3 + 1] = H; xs[e * 3 + 1] = Ly.h1 + e * BH; ldx[e * 3 + 1] = H;
      dz[e * 3 + 2] = Ly.dze3 + e * H; ldz[e * 3 + 2] = MH; xs[e * 3 + 2] = Ly.h2 + e * BH; ldx[e * 3 + 2] = H;
    }
    dz[Pr.A0] = Ly.dza1; ldz[Pr.A0] = H; xs[Pr.A0] = x_att; ldx[Pr.A0] = MH;
    dz[Pr.A0 + 1] = Ly.dza2; ldz[Pr.A0 + 1] = H; xs[Pr.A0 + 1] = Ly.a1; ldx[Pr.A0 + 1] = H;
    dz[Pr.A0 + 2] = Ly.dza3; ldz[Pr.A0 + 2] = H; xs[Pr.A0 + 2] = Ly.a2; ldx[Pr.A0 + 2] = H;
    dz[Pr.FA] = Ly.datt; ldz[Pr.FA] = M; xs[Pr.FA] = Ly.a3; ldx[Pr.FA] = H;
    dz[Pr.O1] = Ly.demo; ldz[Pr.O1] = C1; xs[Pr.O1] = Ly.feat; ldx[Pr.O1] = H;
    dz[Pr.O2] = Ly.dval; ldz[Pr.O2] = C2; xs[Pr.O2] = Ly.feat; ldx[Pr.O2] = H;
    const int nlin = C2 ? Pr.nlin : Pr.nlin - 1;   // fc_out_2 is empty when C2 = 0
    {
      TgBase dw;
      dw.a = ws; dw.a_gs = S; dw.w = ws; dw.w_gs = S; dw.c = grd; dw.c_gs = P; dw.gate = ws; dw.gate_gs = S;
      dw.rows = 2; dw.act = MER_ACT_NONE; dw.accumulate = 0; dw.ldg = 0;
      TgGemmList L;
      L.np = nlin;
      for (int l = 0; l < nlin; ++l) L.p[l] = tg_prob(dz[l], ldz[l], xs[l], ldx[l], Pr.w[l], Pr.in[l], Pr.out[l], Pr.in[l], B);
      tg_gemm<true, true>(ctx, dw, L, st);
    }
    {
      TgSumList L;
      L.np = nlin;
      int blks = 0;
      for (int l = 0; l < nlin; ++l) {
        TgSum& s = L.p[l];
        s.x = dz[l]; s.ldx = ldz[l]; s.out = Pr.b[l]; s.N = Pr.out[l]; s.blk0 = blks; s.pad = 0;
        blks += (int)cdiv(s.N, 64);
      }
      tg_colsum_kernel<<<dim3(blks, G), 64, 0, st>>>(ctx, ws, S, grd, P, L);
    }
    long long nb = cdiv(P, 256);
    nb = nb < 1 ? 1 : (nb > 1024 ? 1024 : nb);
    tg_adam_kernel<<<dim3((unsigned)nb, G), 256, 0, st>>>(ctx, par, grd, d->adam_m, d->adam_v, P, d->lr, d->weight_decay, d->grad_clip,
                                                          d->beta1, d->beta2, d->eps, d->step);
  }
  tg_finish_kernel<<<1, 256, 0, st>>>(ctx, d->step, train, d->cursor);
  return check_launch(fn);
}

extern "C" int mer_fusion_topn_group_step(const mer_fusion_topn_group* d, int train, mer_stream_t stream) {
  return tg_step("mer_fusion_topn_group_step", d, 27, train, stream);
}

static int tg_mask(const char* fn, int site_shift, uint64_t seed, int step, int site, int rows, int cols, float p, uint8_t* keep,
                   mer_stream_t stream) {
  tg_mask_kernel<<<(unsigned)cdiv((long long)rows * cols, 256), 256, 0, (hipStream_t)stream>>>(seed, step, site, rows, cols, p, keep,
                                                                                               site_shift);
  return check_launch(fn);
}

extern "C" int mer_fusion_topn_group_dropout_mask(uint64_t seed, int step, int site, int rows, int cols, float p, uint8_t* keep,
                                                  mer_stream_t stream) {
  MER_REQUIRE(keep && rows > 0 && cols > 0 && rows <= TG_MAXB && cols < 65536 && site >= 0 && site <= TG_MAXS, MER_EINVAL,
              "mer_fusion_topn_group_dropout_mask: bad args (rows=%d cols=%d site=%d)", rows, cols, site);
  return tg_mask("mer_fusion_topn_group_dropout_mask", 27, seed, step, site, rows, cols, p, keep, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// the 3-stream ABI (mer_fusion_group_*): the engine with M = 3 (audio, text, video), C2 = 1 and the site << 30 counter layout.
// For M = 3 tg_params is model.parameters() order of the Attention model and tg_layout the workspace this ABI always had.
// ---------------------------------------------------------------------------------------------------------------------
static int fg_as_topn(const char* fn, const mer_fusion_group* d, mer_fusion_topn_group* t) {
  MER_REQUIRE(d, MER_EINVAL, "%s: null descriptor", fn);
  MER_REQUIRE(d->G > 0 && d->B > 0 && d->B <= TG_MAXB && d->n_steps > 0, MER_ESHAPE,
              "%s: need G > 0, 0 < B <= %d, n_steps > 0 (G=%d B=%d n_steps=%d)", fn, TG_MAXB, d->G, d->B, d->n_steps);
  MER_REQUIRE(d->Da > 0 && d->Dt > 0 && d->Dv > 0 && d->H > 0 && d->Da < 65536 && d->Dt < 65536 && d->Dv < 65536 && 3 * d->H < 65536,
              MER_ESHAPE, "%s: bad dims Da=%d Dt=%d Dv=%d H=%d", fn, d->Da, d->Dt, d->Dv, d->H);
  MER_REQUIRE(d->C1 > 0 && d->C1 <= 64 && d->C2 == 1, MER_EUNSUPPORTED,
              "%s: only the emotion (C1 <= 64) + valence (C2 = 1) heads are built (C1=%d C2=%d)", fn, d->C1, d->C2);
  *t = mer_fusion_topn_group{};
  t->G = d->G; t->B = d->B; t->n_steps = d->n_steps; t->M = 3; t->H = d->H; t->C1 = d->C1; t->C2 = d->C2; t->P = d->P;
  t->D[0] = d->Da; t->D[1] = d->Dt; t->D[2] = d->Dv;
  t->feat[0] = d->feat_a; t->feat[1] = d->feat_t; t->feat[2] = d->feat_v;
  t->params = d->params; t->grads = d->grads; t->adam_m = d->adam_m; t->adam_v = d->adam_v; t->step = d->step;
  t->lr = d->lr; t->weight_decay = d->weight_decay; t->grad_clip = d->grad_clip; t->dropout = d->dropout; t->seed = d->seed;
  t->beta1 = d->beta1; t->beta2 = d->beta2; t->eps = d->eps;
  t->emo = d->emo; t->val = d->val; t->n_rows = d->n_rows; t->index = d->index; t->count = d->count; t->cursor = d->cursor;
  t->out_loss = d->out_loss; t->out_emo = d->out_emo; t->out_val = d->out_val;
  t->workspace = d->workspace; t->workspace_bytes = d->workspace_bytes;
  return MER_OK;
}

extern "C" long long mer_fusion_group_param_count(int Da, int Dt, int Dv, int H, int C1, int C2) {
  if (Da <= 0 || Dt <= 0 || Dv <= 0 || H <= 0 || C1 <= 0 || C2 <= 0) return MER_EINVAL;
  const int D[3] = {Da, Dt, Dv};
  return tg_params(3, D, H, C1, C2).P;
}

extern "C" long long mer_fusion_group_workspace_bytes(const mer_fusion_group* d) {
  mer_fusion_topn_group t;
  const int rc = fg_as_topn("mer_fusion_group_workspace_bytes", d, &t);
  return rc != MER_OK ? rc : (long long)t.G * tg_layout(t).stride * (long long)sizeof(float);
}

extern "C" int mer_fusion_group_step(const mer_fusion_group* d, int train, mer_stream_t stream) {
  mer_fusion_topn_group t;
  const int rc = fg_as_topn("mer_fusion_group_step", d, &t);
  return rc != MER_OK ? rc : tg_step("mer_fusion_group_step", &t, 30, train, stream);
}

extern "C" int mer_fusion_group_dropout_mask(uint64_t seed, int step, int site, int rows, int cols, float p, uint8_t* keep,
                                             mer_stream_t stream) {
  MER_REQUIRE(keep && rows > 0 && cols > 0 && rows <= 16384 && cols < 65536 && site >= 0 && site < 4, MER_EINVAL,
              "mer_fusion_group_dropout_mask: bad args (rows=%d cols=%d site=%d)", rows, cols, site);
  return tg_mask("mer_fusion_group_dropout_mask", 30, seed, step, site, rows, cols, p, keep, stream);
}
