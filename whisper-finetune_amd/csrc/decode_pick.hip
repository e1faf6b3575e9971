// decode_pick.hip — what a decoding step does with a logits row, and the embedding that starts the next step (include/wft.h
// "Greedy decoding", "Timestamp rules", "Sampled decoding").
//
//  decode_embed_kernel                       token + positional embedding at the device-side position
//  decode_pick_kernel<TS, SAMPLE>           suppress, arg-max, log-probability, state update.  TS: under upstream's timestamp rules;
//                                            SAMPLE: a temperature per row, Gumbel-max over Philox noise.  One kernel template,
//                                            the four instantiations behind wft_decode_pick / _pick_ts / _sample / _sample_ts.
//  decode_count_kernel                       the unfinished-row count behind a pick or a beam-search step
#include "decode_common.h"

// ----------------------------------------------------------------------------- embedding at the device-side position
// out[b] = emb[tokens[b, len[b] - 1]] + pos[len[b] - 1]: the arithmetic of embed_fwd_kernel (embed.hip), one fp32 add and one rounding.
__global__ __launch_bounds__(256) void decode_embed_kernel(const long* tokens, long ld_tokens, const int* len, const float* emb,
                                                            const float* pos, unsigned short* out, int B, int n_ctx, int d, long V) {
  const int dv = d >> 3;
  const long total = (long)B * dv;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int b = (int)(i / dv);
    const int c = (int)(i - (long)b * dv) * 8;
    int p = len[b] - 1;
    p = p < 0 ? 0 : (p >= n_ctx ? n_ctx - 1 : p);
    long tok = tokens[(long)b * ld_tokens + p];
    tok = tok < 0 ? 0 : (tok >= V ? V - 1 : tok);
    const float* e = emb + tok * d + c;
    const float* pp = pos + (long)p * d + c;
    const f32x4 a0 = *(const f32x4*)e, a1 = *(const f32x4*)(e + 4);
    const f32x4 b0 = *(const f32x4*)pp, b1 = *(const f32x4*)(pp + 4);
    u32x4 o = {pack2bf(a0[0] + b0[0], a0[1] + b0[1]), pack2bf(a0[2] + b0[2], a0[3] + b0[3]),
               pack2bf(a1[0] + b1[0], a1[1] + b1[1]), pack2bf(a1[2] + b1[2], a1[3] + b1[3])};
    *(u32x4*)(out + (long)b * d + c) = o;
  }
}

extern "C" int wft_decode_embed(const int64_t* tokens, int64_t ld_tokens, const int32_t* len, const float* emb, const float* pos,
                                wft_bf16* out, int B, int n_ctx, int d, int64_t V, void* stream) {
  WFT_CHECK_ARG(tokens && len && emb && pos && out, "null pointer");
  WFT_CHECK_ARG(B >= 1 && n_ctx >= 1 && ld_tokens >= n_ctx && d >= 8 && d % 8 == 0 && V >= 1, "bad shape");
  WFT_CHECK_ARG(((((uintptr_t)emb) | ((uintptr_t)pos) | ((uintptr_t)out)) & 15) == 0, "16-byte alignment");
  const long total = (long)B * (d / 8);
  const unsigned grid = (unsigned)((total + 255) / 256 > 1024 ? 1024 : (total + 255) / 256);
  hipLaunchKernelGGL(decode_embed_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const long*)tokens, (long)ld_tokens, len, emb, pos,
                     out, B, n_ctx, d, (long)V);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- the unfinished-row count
__global__ __launch_bounds__(256) void decode_count_kernel(const int* finished, int B, int* unfinished) {
  __shared__ int s[4];
  int n = 0;
  for (int i = threadIdx.x; i < B; i += 256) n += finished[i] ? 0 : 1;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) unfinished[0] = s[0] + s[1] + s[2] + s[3];
}

void wft_decode_count_launch(const int* finished, int B, int* unfinished, hipStream_t s) {
  hipLaunchKernelGGL(decode_count_kernel, dim3(1), dim3(256), 0, s, finished, B, unfinished);
}

// ----------------------------------------------------------------------------- the noise of the sampled pick
// The noise is a pure function of (seed[r], len[r], col): Philox4x32-10 keyed by the seed, counter (col >> 2, len, 0, 0), output
// word col & 3; one block serves the 4 columns of a lane's 16-byte read half, so a lane runs 2 blocks per 8 columns (kept in
// registers across the calls of pick_scan's f).
struct philox4 {
  unsigned w[4];
};

__host__ __device__ __forceinline__ unsigned philox_mulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }

__host__ __device__ __forceinline__ philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = philox_mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned h1 = philox_mulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return philox4{{c0, c1, c2, c3}};
}

// g = -log(-log(v)), v = (2k + 1) * 2^-24 with k the word's top 23 bits: an odd 24-bit integer scaled, exact in fp32 and inside
// (0, 1).  The accurate logf: the winners are the columns with v near 1, where -log(v) ~ 1 - v is tiny and __logf's absolute error
// would be a large relative one.
__device__ __forceinline__ float gumbel_of(unsigned word) {
  const float v = (float)(2u * (word >> 9) + 1u) * 5.9604644775390625e-08f;
  return -logf(-logf(v));
}

// the per-row noise source: g(col), one Philox block per 4 columns, the last block kept
struct gumbel_row {
  unsigned k0, k1, pos;
  int blk;
  philox4 cur;
  __device__ __forceinline__ float operator()(int col) {
    if ((col >> 2) != blk) {
      blk = col >> 2;
      cur = philox4x32_10((unsigned)blk, pos, 0u, 0u, k0, k1);
    }
    const int j = col & 3;
    const unsigned w = j == 0 ? cur.w[0] : (j == 1 ? cur.w[1] : (j == 2 ? cur.w[2] : cur.w[3]));
    return gumbel_of(w);
  }
};

// the logit of the workgroup's winning key column `bi` in every thread: the thread that brought (mine_i == bi) publishes the logit
// it carried.  s_x: used by nothing else.
__device__ __forceinline__ float sample_wg_logit(int bi, int mine_i, float mine_x, float* s_x) {
  if (bi != PICK_NONE && mine_i == bi) *s_x = mine_x;
  __syncthreads();
  return bi != PICK_NONE ? *s_x : -INFINITY;
}

// ----------------------------------------------------------------------------- the pick: greedy and sampled, plain and timestamp form
// One workgroup per state row.  Pass 1: maximum of the un-suppressed logits with its LOWEST index (each thread scans its columns in
// ascending order with a strict compare; the tree compares (value, index) pairs).  Pass 2 (the row is L2-resident): sum of
// exp(x - max) over the same columns, so log p(pick) = -log(sum).  Thread 0 then advances the row's state unless it is finished.
// TS: the timestamp-rule form.  The timestamps win -> the best timestamp column under the normaliser sum_ts; otherwise the better of
// the two pairs (value descending, the lower column on ties) under sum_ts + sum_text.
// SAMPLE: one more question per row (include/wft.h "Sampled decoding"): t = temperature[r] > 0 draws the token by the Gumbel-max
// rule — the arg-max of key(col) = x[col] / t + g(col) over the live columns is a draw from softmax(x / t) — and t <= 0 takes the
// greedy statements of this kernel (same scans, same reduction order: same bits).  State row r reads logits row r / group.  Plain
// form: the key scan rides the max pass (one HBM read of the row), the sum pass is the greedy one.  TS form: ts_decide's two passes
// on the UNTEMPERED row (upstream filters before GreedyDecoder.update divides by the temperature), then — t > 0 only — one more scan
// of the L2-resident row under the final predicate, as decode_topk_kernel<true> does; the log-probability reuses ts_decide's maximum
// and sums.  Either way it is the pick's log-softmax at temperature 1 over the live columns.
// Without SAMPLE temperature / seed / group are not read (the launch passes null), and s_x and the noise source go with the draw.
// Why one __global__ template and not two kernels around a shared __device__ body: the extra inlining level changes the instruction
// streams of three of the four forms (by value or by reference alike), this form changes none but one: with five parameters hipcc
// fetches three kernel-argument words of the <TS, greedy> form in one s_load_dwordx4 where the two-parameter kernel, whose argument
// segment ended inside that read, needed two loads.
template <bool TS, bool SAMPLE>
__global__ __launch_bounds__(PICK_THREADS) void decode_pick_kernel(wft_decode_pick_args a, wft_ts_rules ru, const float* temperature,
                                                                   const unsigned long long* seed, int group) {
  __shared__ float s_v[PICK_WAVES];
  __shared__ int s_i[PICK_WAVES];
  __shared__ float s_sum[PICK_WAVES];
  __shared__ float s_x;
  const int b = blockIdx.x;
  const unsigned short* row = a.logits + (long)(SAMPLE ? b / group : b) * a.ld;
  const int V = (int)a.V;
  const int L = a.len[b];
  const unsigned char* m1 = a.suppress;
  const unsigned char* m2 = (a.suppress_first && a.first_len && L == a.first_len[b]) ? a.suppress_first : nullptr;
  const float temp = SAMPLE ? temperature[b] : 0.f;
  const bool draw = SAMPLE && temp > 0.f;
  const float inv_t = draw ? 1.0f / temp : 0.f;
  const unsigned long long sd = SAMPLE ? seed[b] : 0;
  gumbel_row g = {(unsigned)sd, (unsigned)(sd >> 32), (unsigned)L, -1, {}};

  float best = -INFINITY;
  int bi = PICK_NONE;
  float lp;
  float kbest = -INFINITY, kx = -INFINITY;  // the best key of this thread's columns, its column and its logit
  int ki = PICK_NONE;
  auto key = [&](float x, int col) {
    const float k = x * inv_t + g(col);
    if (k > kbest) {  // (strict, ascending columns: a tie stays with the lower column; a -inf logit never enters)
      kbest = k;
      ki = col;
      kx = x;
    }
  };
  if constexpr (TS) {
    __shared__ int s_ts[PICK_WAVES];
    __shared__ float s_sum2[PICK_WAVES];
    ts_row t = ts_row_rules(ru, a.tokens + (long)b * a.ld_tokens, a.ld_tokens, a.first_len[b], L, V, a.eot, s_ts);
    const ts_pass p = ts_decide(row, V, m1, m2, t.ts_begin, [&](int col) { return ts_live(t, col); }, s_v, s_i, s_sum, s_sum2);
    if (draw) {
      if (p.wins) t.text_lo = t.ts_begin;
      pick_scan(row, V, m1, m2, [&](int col) { return ts_live(t, col); }, key);
      const int mine = ki;
      __syncthreads();
      pick_wg_best(kbest, ki, s_v, s_i);
      bi = ki;
      best = sample_wg_logit(bi, mine, kx, &s_x);
      lp = (best - p.m) - __logf(p.wins ? p.ss : p.st + p.ss);
    } else {
      const bool ts = p.wins || pick_better(p.bs, p.is, p.bt, p.it);
      best = ts ? p.bs : p.bt;
      bi = ts ? p.is : p.it;
      lp = p.wins ? (p.bs - p.m) - __logf(p.ss) : -__logf(p.st + p.ss);
    }
  } else {
    if (draw) {
      pick_scan(row, V, m1, m2, pick_all{}, [&](float x, int col) {
        if (x > best) {
          best = x;
          bi = col;
        }
        key(x, col);
      });
    } else {
      pick_scan(row, V, m1, m2, pick_all{}, [&](float x, int col) {
        if (x > best) {
          best = x;
          bi = col;
        }
      });
    }
    pick_wg_best(best, bi, s_v, s_i);
    if (draw) {
      const int mine = ki;
      __syncthreads();
      pick_wg_best(kbest, ki, s_v, s_i);
      const float x = sample_wg_logit(ki, mine, kx, &s_x);
      const float sum = pick_wg_sumexp(row, V, m1, m2, best, bi != PICK_NONE, s_sum);
      lp = (x - best) - __logf(sum);
      bi = ki;
    } else {
      lp = -__logf(pick_wg_sumexp(row, V, m1, m2, best, bi != PICK_NONE, s_sum));
    }
  }
  const bool any = bi != PICK_NONE;
  if (threadIdx.x == 0) {
    const long pick = any ? bi : a.eot;  // (every column suppressed: the row ends)
    if (!any) lp = 0.f;
    if (a.pick_out) a.pick_out[b] = pick;
    if (a.logprob_out) a.logprob_out[b] = lp;
    if (!a.finished[b]) {  // a finished row is frozen
      if (L >= 0 && L < a.max_len) {
        a.tokens[(long)b * a.ld_tokens + L] = pick;
        a.sum_logprob[b] += lp;
        a.len[b] = L + 1;
      }
      a.finished[b] = (pick == a.eot || L + 1 >= a.max_len) ? 1 : 0;
    }
  }
}

static int pick_check(const wft_decode_pick_args* a, const char* who) {
  WFT_CHECK_ARG_AS(who, a && a->logits && a->tokens && a->len && a->finished && a->sum_logprob && a->unfinished, "null pointer");
  WFT_CHECK_ARG_AS(who, a->B >= 1 && a->V >= 1 && a->V <= 0x7ffffff0L, "bad shape");
  WFT_CHECK_ARG_AS(who, a->ld % 8 == 0 && a->ld >= (a->V + 7) / 8 * 8 && (((uintptr_t)a->logits) & 15) == 0, "logits rows: 16-byte aligned, ld >= V rounded up to 8");
  WFT_CHECK_ARG_AS(who, a->max_len >= 1 && a->max_len <= a->ld_tokens, "max_len must fit the token buffer");
  WFT_CHECK_ARG_AS(who, a->eot >= 0 && a->eot < a->V, "eot outside the vocabulary");
  WFT_CHECK_ARG_AS(who, !a->suppress_first || a->first_len, "suppress_first needs first_len");
  return WFT_OK;
}

static int sample_check(const wft_decode_pick_args* a, const wft_sample_rules* s, const char* who) {
  WFT_CHECK_ARG_AS(who, s && s->temperature && s->seed, "null pointer (temperature / seed)");
  WFT_CHECK_ARG_AS(who, s->group >= 1 && a->B % s->group == 0, "group must be >= 1 and divide the state rows");
  return WFT_OK;
}

// the four entry points: the checks in their order (state, sampling rules, timestamp rules), the kernel of the form, the count
template <bool TS, bool SAMPLE>
static int pick_launch(const wft_decode_pick_args* a, const wft_sample_rules* s, const wft_ts_rules* ru, const char* who, void* stream) {
  if (int rc = pick_check(a, who)) return rc;
  if constexpr (SAMPLE)
    if (int rc = sample_check(a, s, who)) return rc;
  if constexpr (TS) {
    if (int rc = ts_check(ru, a->eot, a->V, who)) return rc;
    WFT_CHECK_ARG_AS(who, a->first_len, "the timestamp rules need first_len");
  }
  const dim3 grid((unsigned)a->B), block(PICK_THREADS);
  hipLaunchKernelGGL((decode_pick_kernel<TS, SAMPLE>), grid, block, 0, (hipStream_t)stream, *a, TS ? *ru : wft_ts_rules{},
                     SAMPLE ? s->temperature : nullptr, SAMPLE ? (const unsigned long long*)s->seed : nullptr, SAMPLE ? s->group : 1);
  wft_decode_count_launch((const int*)a->finished, a->B, a->unfinished, (hipStream_t)stream);
  WFT_CHECK_LAUNCH_AS(who);
  return WFT_OK;
}

extern "C" int wft_decode_pick(const wft_decode_pick_args* a, void* stream) { return pick_launch<false, false>(a, nullptr, nullptr, __func__, stream); }
extern "C" int wft_decode_pick_ts(const wft_decode_pick_args* a, const wft_ts_rules* ru, void* stream) {
  return pick_launch<true, false>(a, nullptr, ru, __func__, stream);
}
extern "C" int wft_decode_sample(const wft_decode_pick_args* a, const wft_sample_rules* s, void* stream) {
  return pick_launch<false, true>(a, s, nullptr, __func__, stream);
}
extern "C" int wft_decode_sample_ts(const wft_decode_pick_args* a, const wft_sample_rules* s, const wft_ts_rules* ru, void* stream) {
  return pick_launch<true, true>(a, s, ru, __func__, stream);
}
