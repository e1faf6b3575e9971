// decode_common.h — what the decoding translation units share (include/wft.h "Greedy decoding", "Beam search", "Timestamp rules",
// "Sampled decoding").  Files: decode_attn.hip (single-token attention, greedy and beam), decode_pick.hip (embedding, the greedy /
// sampled pick, the unfinished-row count), decode_beam.hip (top-(W + 1) candidates, the beam-search step).
//  dec_unpack8                                      8 bf16 of a 16-byte read as floats: every file
//  PICK_*, pick_scan, pick_wg_best / _sum / _sumexp  the masked row scan and the workgroup reduces: decode_pick.hip, decode_beam.hip
//  ts_row_rules, ts_decide, ts_check                the timestamp rules, device and argument check: the _ts forms of both files
//  wft_decode_count_launch (decode_pick.hip)        enqueues decode_count_kernel: the pick / sample entry points, wft_beam_update
#pragma once
#include "common.h"

__device__ __forceinline__ void dec_unpack8(const u32x4 r, float* f) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __builtin_bit_cast(float, r[i] << 16);
    f[2 * i + 1] = __builtin_bit_cast(float, r[i] & 0xffff0000u);
  }
}

// unfinished[0] = the number of zero entries of finished[0..B): one workgroup, behind the kernel that wrote `finished`
void wft_decode_count_launch(const int* finished, int B, int* unfinished, hipStream_t s);

// ----------------------------------------------------------------------------- the row scan and the workgroup reduces
// One workgroup per logits row; what decode_pick_kernel / decode_sample_kernel and decode_topk_kernel are made of.
#define PICK_THREADS 256
#define PICK_WAVES (PICK_THREADS / 64)
#define PICK_NONE 0x7fffffff

__device__ __forceinline__ bool pick_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// f(x, col) for the live columns of a logits row — col < V, live(col), neither mask set — that this thread owns: 16-byte reads,
// ascending columns.  live: the per-row column predicate of the timestamp rules (ts_live below), pick_all where there are none.
struct pick_all {
  __device__ __forceinline__ bool operator()(int) const { return true; }
};

template <typename P, typename F>
__device__ __forceinline__ void pick_scan(const unsigned short* row, int V, const unsigned char* m1, const unsigned char* m2, P live, F f) {
  for (int c0 = threadIdx.x * 8; c0 < V; c0 += PICK_THREADS * 8) {
    float x[8];
    dec_unpack8(*(const u32x4*)(row + c0), x);  // (ld % 8 == 0 and ld >= V rounded up to 8: in bounds)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = c0 + j;
      if (col < V && live(col) && !(m1 && m1[col]) && !(m2 && m2[col])) f(x[j], col);
    }
  }
}

// the workgroup's best (value, lowest index) in every thread: the wave butterfly, then the waves in wave order.  s_v / s_i: one
// entry per wave; the caller puts a barrier between two calls.
__device__ __forceinline__ void pick_wg_best(float& best, int& bi, float* s_v, int* s_i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (pick_better(ov, oi, best, bi)) {
      best = ov;
      bi = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    s_v[threadIdx.x >> 6] = best;
    s_i[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  best = s_v[0];
  bi = s_i[0];
  for (int w = 1; w < PICK_WAVES; ++w)
    if (pick_better(s_v[w], s_i[w], best, bi)) {
      best = s_v[w];
      bi = s_i[w];
    }
}

// the workgroup's sum of `sum` in every thread: the wave butterfly, then the waves in wave order.  s_sum: one entry per wave, not
// reused without a barrier in between.
__device__ __forceinline__ float pick_wg_sum(float sum, float* s_sum) {
  sum = wave_sum(sum);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  float tot = s_sum[0];
  for (int w = 1; w < PICK_WAVES; ++w) tot += s_sum[w];
  return tot;
}

// sum of exp(x - top) over the live columns of the row (0 when `any` is false), in every thread: per thread in column order, then
// pick_wg_sum
__device__ __forceinline__ float pick_wg_sumexp(const unsigned short* row, int V, const unsigned char* m1, const unsigned char* m2, float top,
                                                bool any, float* s_sum) {
  float sum = 0.f;
  if (any) pick_scan(row, V, m1, m2, pick_all{}, [&](float x, int) { sum += __expf(x - top); });
  return pick_wg_sum(sum, s_sum);
}

// ----------------------------------------------------------------------------- the timestamp rules (include/wft.h "Timestamp rules")
// Upstream's `ApplyTimestampRules`, restated.  Rules 1-4 remove column RANGES that follow from three facts about the row's sampled
// tokens tokens[r, F..L) — the last one, the one before it, the last timestamp among them — so they become four per-row scalars and
// a live column is `col != no_ts && (col < ts_begin ? col >= text_lo : ts_lo <= col <= ts_hi)`:
//   1  no_ts is removed                                                                       (no_ts = -1: nothing)
//   2  last_ts && pen_ts: every timestamp is removed (ts_lo = V); last_ts && !pen_ts: columns 0..eot-1 are (text_lo = eot)
//   3  t = the last sampled timestamp: ts_begin..t-1 are removed, and t itself unless last_ts && !pen_ts  (ts_lo = t or t + 1)
//   4  no sampled token yet: all text is removed (text_lo = ts_begin), and timestamps above ts_begin + max_initial (ts_hi)
// Rule 5 (the probability rule) needs the row's values and lives in the kernels: ts_decide below.
// The facts are read from `tokens` by the workgroup itself — at most n_text_ctx i64 values, one strided read and a max-index
// reduce — so there is no per-row rule state to keep, permute or reset, and nothing on the host depends on the step.
struct ts_row {
  int no_ts, ts_begin, text_lo, ts_lo, ts_hi;
};

__device__ __forceinline__ bool ts_live(const ts_row& t, int col) {
  return col != t.no_ts && (col < t.ts_begin ? col >= t.text_lo : (col >= t.ts_lo && col <= t.ts_hi));
}

// the same ts_row in every thread.  tok: the row's tokens (ld_tokens of them are addressable), F / L: first_len / len of the row;
// s_ts: one entry per wave, used by nothing else.
__device__ __forceinline__ ts_row ts_row_rules(const wft_ts_rules& ru, const long* tok, long ld_tokens, int F, int L, int V, int eot,
                                               int* s_ts) {
  L = (int)min((long)max(L, 0), ld_tokens);
  F = min(max(F, 0), L);
  const int n = L - F;  // sampled tokens
  int idx = -1;         // position of the last sampled timestamp (ascending positions per thread: the last hit is its largest)
  for (int i = F + (int)threadIdx.x; i < L; i += PICK_THREADS)
    if (tok[i] >= ru.ts_begin) idx = i;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) idx = max(idx, __shfl_xor(idx, o, 64));
  if ((threadIdx.x & 63) == 0) s_ts[threadIdx.x >> 6] = idx;
  __syncthreads();
  idx = s_ts[0];
  for (int w = 1; w < PICK_WAVES; ++w) idx = max(idx, s_ts[w]);
  const bool last_ts = n >= 1 && tok[L - 1] >= ru.ts_begin;
  const bool pen_ts = n < 2 || tok[L - 2] >= ru.ts_begin;
  ts_row t;
  t.no_ts = ru.no_timestamps;
  t.ts_begin = ru.ts_begin;
  t.text_lo = 0;
  t.ts_lo = ru.ts_begin;
  t.ts_hi = V - 1;
  if (last_ts && pen_ts) t.ts_lo = V;
  if (last_ts && !pen_ts) t.text_lo = eot;
  if (idx >= 0) {
    const long last = min(tok[idx], (long)V - 1);
    t.ts_lo = max(t.ts_lo, (int)last + ((last_ts && !pen_ts) ? 0 : 1));
  }
  if (n == 0) {
    t.text_lo = ru.ts_begin;
    if (ru.max_initial >= 0) t.ts_hi = (int)min((long)V - 1, (long)ru.ts_begin + ru.max_initial);
  }
  return t;
}

// Rule 5 rides the two passes the kernels make anyway.  Pass 1 keeps TWO arg-best pairs, the best live text column (bt, it) and the
// best live timestamp column (bs, is); pass 2 keeps two sums of exp(x - m), m = max(bt, bs), per thread in column order and reduced
// by pick_wg_sum.  Both log-probabilities share the normaliser, so "logsumexp of the timestamps > the best text log-probability"
// is log(sum_ts) > bt - m (an empty side is -inf: 0 timestamps never win, 0 text columns always lose to a live timestamp).
struct ts_pass {
  float bt, bs, m, st, ss;
  int it, is;
  bool wins;  // the timestamps win: every text column is removed
};

template <typename P>
__device__ __forceinline__ ts_pass ts_decide(const unsigned short* row, int V, const unsigned char* m1, const unsigned char* m2, int ts_begin,
                                             P live, float* s_v, int* s_i, float* s_sum, float* s_sum2) {
  ts_pass p;
  p.bt = p.bs = -INFINITY;
  p.it = p.is = PICK_NONE;
  pick_scan(row, V, m1, m2, live, [&](float x, int col) {
    if (col < ts_begin) {
      if (x > p.bt) {
        p.bt = x;
        p.it = col;
      }
    } else if (x > p.bs) {
      p.bs = x;
      p.is = col;
    }
  });
  pick_wg_best(p.bt, p.it, s_v, s_i);
  __syncthreads();
  pick_wg_best(p.bs, p.is, s_v, s_i);
  p.m = fmaxf(p.bt, p.bs);
  p.st = p.ss = 0.f;
  if (p.it != PICK_NONE || p.is != PICK_NONE) {
    const float m = p.m;
    pick_scan(row, V, m1, m2, live, [&](float x, int col) {
      const float e = __expf(x - m);
      if (col < ts_begin) p.st += e;
      else p.ss += e;
    });
  }
  p.st = pick_wg_sum(p.st, s_sum);
  p.ss = pick_wg_sum(p.ss, s_sum2);
  p.wins = __logf(p.ss) > p.bt - p.m;
  return p;
}

// the rule constants against the row's vocabulary (`who`: the entry point that reports)
static inline int ts_check(const wft_ts_rules* ru, int eot, int64_t V, const char* who) {
  WFT_CHECK_ARG_AS(who, ru, "null pointer");
  WFT_CHECK_ARG_AS(who, ru->ts_begin > eot && ru->ts_begin < V, "ts_begin must lie in (eot, V)");
  WFT_CHECK_ARG_AS(who, ru->no_timestamps >= -1 && ru->no_timestamps < V, "no_timestamps is -1 or a column");
  return WFT_OK;
}
