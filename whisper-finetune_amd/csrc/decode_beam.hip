// decode_beam.hip — the kernels of a beam-search step (include/wft.h "Beam search").
//
//  decode_topk_kernel<TS>   the W + 1 best continuations per hypothesis, plain or under the timestamp rules: the row scan, the
//                           reduces and the rules of the pick (decode_common.h)
//  beam_update_kernel       one beam-search step per audio on the device-side state
#include "decode_common.h"

// ----------------------------------------------------------------------------- the W + 1 best continuations of a row
// One workgroup per logits row, decode_pick_kernel's 16-byte row reads and masks (pick_scan).  Pass 1: every thread keeps the TOPK_MAX best
// (value, column) of ITS columns as a sorted list in registers (columns come in ascending order, so a tie stays behind the lower
// column).  Merge: k rounds, each the workgroup's best list head under (value desc, column asc) — a fixed-order tree, no atomics —
// after which the one thread that owns that column pops it.  Pass 2 (the row is L2-resident): decode_pick_kernel's sum of
// exp(x - max), in its order; log p = (x - max) - log(sum).  A live column whose logit is -inf can never be a candidate.
#define TOPK_MAX 9

// TS: the timestamp-rule form (wft_decode_topk_ts).  Rule 5 decides which columns are live, so it must precede the candidate
// merge: ts_decide's two passes run first (the first one reads HBM, the second the L2-resident row), then the list pass above runs
// unchanged under the FINAL predicate — a third scan, of a row that is still L2-resident — and the log-probabilities reuse
// ts_decide's maximum and sums.  Chosen over two register lists per thread (text / timestamp, merged by rule 5's outcome): the
// list insertion, the merge rounds and the pop stay the code of the plain kernel and 2 x 9 more (value, column) registers are not
// held through the scan.  Neither form has been timed (DESIGN.md §3 "Timestamp rules").
template <bool TS>
__global__ __launch_bounds__(PICK_THREADS) void decode_topk_kernel(wft_decode_topk_args a, wft_ts_rules ru, const long* tokens, long ld_tokens,
                                                                   int eot) {
  __shared__ float s_v[PICK_WAVES];
  __shared__ int s_i[PICK_WAVES];
  __shared__ float s_sum[PICK_WAVES];
  __shared__ float s_wv[TOPK_MAX];
  __shared__ int s_wi[TOPK_MAX];
  const int tid = threadIdx.x;
  const long r = (long)blockIdx.x * a.row_step;
  const unsigned short* row = a.logits + (long)blockIdx.x * a.ld;
  const int V = (int)a.V;
  const unsigned char* m1 = a.suppress;
  const unsigned char* m2 = (a.suppress_first && a.first_len && a.len && a.len[r] == a.first_len[r]) ? a.suppress_first : nullptr;

  ts_row t = {};
  float top = 0.f, tot = 0.f;
  auto live = [&](int col) {
    if constexpr (TS) return ts_live(t, col);
    else return true;
  };
  if constexpr (TS) {
    __shared__ int s_ts[PICK_WAVES];
    __shared__ float s_sum2[PICK_WAVES];
    t = ts_row_rules(ru, tokens + r * ld_tokens, ld_tokens, a.first_len[r], a.len[r], V, eot, s_ts);
    const ts_pass p = ts_decide(row, V, m1, m2, t.ts_begin, live, s_v, s_i, s_sum, s_sum2);
    if (p.wins) t.text_lo = t.ts_begin;
    top = p.m;
    tot = p.wins ? p.ss : p.st + p.ss;
  }

  float lv[TOPK_MAX];
  int li[TOPK_MAX];
#pragma unroll
  for (int p = 0; p < TOPK_MAX; ++p) {
    lv[p] = -INFINITY;
    li[p] = PICK_NONE;
  }
  pick_scan(row, V, m1, m2, live, [&](float x, int col) {
    if (x > lv[TOPK_MAX - 1]) {
      lv[TOPK_MAX - 1] = x;
      li[TOPK_MAX - 1] = col;
#pragma unroll
      for (int p = TOPK_MAX - 1; p > 0; --p) {
        if (lv[p] > lv[p - 1]) {  // strict: an equal value stays behind the earlier (lower) column
          const float tv = lv[p]; lv[p] = lv[p - 1]; lv[p - 1] = tv;
          const int ti = li[p]; li[p] = li[p - 1]; li[p - 1] = ti;
        }
      }
    }
  });

  for (int rnd = 0; rnd < a.k; ++rnd) {
    float best = lv[0];
    int bi = li[0];
    pick_wg_best(best, bi, s_v, s_i);
    if (bi != PICK_NONE && li[0] == bi) {  // the owner of that column pops it
#pragma unroll
      for (int p = 0; p < TOPK_MAX - 1; ++p) {
        lv[p] = lv[p + 1];
        li[p] = li[p + 1];
      }
      lv[TOPK_MAX - 1] = -INFINITY;
      li[TOPK_MAX - 1] = PICK_NONE;
    }
    if (tid == 0) {
      s_wv[rnd] = best;
      s_wi[rnd] = bi;
    }
    __syncthreads();
  }
  if constexpr (!TS) {
    top = s_wv[0];
    tot = pick_wg_sumexp(row, V, m1, m2, top, s_wi[0] != PICK_NONE, s_sum);
  }
  if (tid < a.k) {
    const bool have = s_wi[tid] != PICK_NONE;
    a.cand_tok[r * a.k + tid] = have ? s_wi[tid] : -1;
    a.cand_logp[r * a.k + tid] = have ? (s_wv[tid] - top) - __logf(tot) : -INFINITY;
  }
}

static int topk_check(const wft_decode_topk_args* a, const char* who) {
  WFT_CHECK_ARG_AS(who, a && a->logits && a->cand_tok && a->cand_logp, "null pointer");
  WFT_CHECK_ARG_AS(who, a->rows >= 1 && a->row_step >= 1 && a->V >= 1 && a->V <= 0x7ffffff0L, "bad shape");
  WFT_CHECK_ARG_AS(who, a->k >= 2 && a->k <= TOPK_MAX, "k = beam size + 1 must lie in 2..9");
  WFT_CHECK_ARG_AS(who, a->ld % 8 == 0 && a->ld >= (a->V + 7) / 8 * 8 && (((uintptr_t)a->logits) & 15) == 0, "logits rows: 16-byte aligned, ld >= V rounded up to 8");
  WFT_CHECK_ARG_AS(who, !a->suppress_first || (a->first_len && a->len), "suppress_first needs len and first_len");
  return WFT_OK;
}

extern "C" int wft_decode_topk(const wft_decode_topk_args* a, void* stream) {
  if (int rc = topk_check(a, __func__)) return rc;
  hipLaunchKernelGGL(decode_topk_kernel<false>, dim3((unsigned)a->rows), dim3(PICK_THREADS), 0, (hipStream_t)stream, *a, wft_ts_rules{},
                     (const long*)nullptr, 0L, 0);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

extern "C" int wft_decode_topk_ts(const wft_decode_topk_args* a, const wft_ts_rules* ru, const int64_t* tokens, int64_t ld_tokens, int eot,
                                  void* stream) {
  if (int rc = topk_check(a, __func__)) return rc;
  WFT_CHECK_ARG(eot >= 0 && eot < a->V, "eot outside the vocabulary");
  if (int rc = ts_check(ru, eot, a->V, __func__)) return rc;
  WFT_CHECK_ARG(a->first_len && a->len, "the timestamp rules need len and first_len");
  WFT_CHECK_ARG(tokens && ld_tokens >= 1, "the timestamp rules need the token rows");
  hipLaunchKernelGGL(decode_topk_kernel<true>, dim3((unsigned)a->rows), dim3(PICK_THREADS), 0, (hipStream_t)stream, *a, *ru,
                     (const long*)tokens, (long)ld_tokens, eot);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}

// ----------------------------------------------------------------------------- one beam-search step per audio
// One workgroup per audio (include/wft.h wft_beam_update).  The <= 72 candidates are ranked by counting, thread 0 walks the order,
// then the rows of `tokens` and `anc` are permuted in place: a permutation of rows touches one column at a time, so the thread that
// owns column t reads its W values into registers and writes them back permuted — no scratch copy, nothing to order between threads.
#define BEAM_MAX_W 8
#define BEAM_THREADS 256
#define BEAM_MAX_CAND (BEAM_MAX_W * (BEAM_MAX_W + 1))

template <typename T>
__device__ __forceinline__ T beam_sel(const T* v, int j) {
  T out = v[0];
#pragma unroll
  for (int i = 1; i < BEAM_MAX_W; ++i) out = j == i ? v[i] : out;
  return out;
}

__global__ __launch_bounds__(BEAM_THREADS) void beam_update_kernel(wft_beam_update_args a) {
  __shared__ float s_score[BEAM_MAX_CAND];
  __shared__ int s_tok[BEAM_MAX_CAND];
  __shared__ int s_order[BEAM_MAX_CAND];
  __shared__ int s_src[BEAM_MAX_W], s_ntok[BEAM_MAX_W], s_fsrc[BEAM_MAX_W];
  __shared__ float s_nscore[BEAM_MAX_W], s_fscore[BEAM_MAX_W];
  __shared__ int s_nfin;
  const int au = blockIdx.x, tid = threadIdx.x, W = a.W, k = W + 1;
  if (a.done[au]) return;  // a done audio is frozen
  const int r0 = au * W;
  const int L = a.len[r0];
  const int have = a.fin_n[au];
  if (L < 1 || L >= a.max_len || have < 0 || have >= a.C) {  // (nothing can be appended: the audio ends here)
    if (tid == 0) a.done[au] = 1;
    return;
  }
  const int nc = (a.first ? 1 : W) * k;
  if (tid < nc) {
    const int j = tid / k, i = tid - j * k;
    const int tok = a.cand_tok[(long)(r0 + j) * k + i];
    float sc = __fadd_rn(a.sum_logprob[r0 + j], a.cand_logp[(long)(r0 + j) * k + i]);
    sc = (tok >= 0 && sc == sc) ? sc : -INFINITY;
    s_tok[tid] = tok;
    s_score[tid] = sc;
  }
  __syncthreads();
  if (tid < nc) {
    const float sc = s_score[tid];
    int rank = 0;
    for (int o = 0; o < nc; ++o) {
      const float so = s_score[o];
      rank += (so > sc || (so == sc && o < tid)) ? 1 : 0;
    }
    s_order[rank] = tid;
  }
  __syncthreads();
  if (tid == 0) {
    int ns = 0, nf = 0;
    for (int p = 0; p < nc && ns < W; ++p) {
      const int cnd = s_order[p], tok = s_tok[cnd], j = cnd / k;
      if (tok < 0) continue;
      if (tok == a.eot) {
        if (have + nf < a.C) {
          s_fsrc[nf] = j;
          s_fscore[nf] = s_score[cnd];
          ++nf;
        }
      } else {
        s_src[ns] = j;
        s_ntok[ns] = tok;
        s_nscore[ns] = s_score[cnd];
        ++ns;
      }
    }
    for (; ns < W; ++ns) {  // (not reached while W non-eot candidates exist, which the host checks)
      s_src[ns] = ns;
      s_ntok[ns] = a.eot;
      s_nscore[ns] = -INFINITY;
    }
    s_nfin = nf;
  }
  __syncthreads();
  const int nf = s_nfin;
  for (int t = tid; t < (int)a.ld_tokens; t += BEAM_THREADS) {
    long v[BEAM_MAX_W];
    int w[BEAM_MAX_W];
#pragma unroll
    for (int j = 0; j < BEAM_MAX_W; ++j) {
      v[j] = (j < W && t < L) ? a.tokens[(long)(r0 + j) * a.ld_tokens + t] : 0;
      w[j] = (j < W && t < L - 1) ? a.anc[(long)(r0 + j) * a.ld_anc + t] : 0;
    }
    for (int e = 0; e < nf; ++e)
      a.fin_tokens[((long)au * a.C + have + e) * a.ld_tokens + t] = t < L ? beam_sel(v, s_fsrc[e]) : (long)a.eot;
    if (t <= L) {
      for (int s = 0; s < W; ++s) {
        const int j = s_src[s];
        a.tokens[(long)(r0 + s) * a.ld_tokens + t] = t < L ? beam_sel(v, j) : (long)s_ntok[s];
        if (t < L) a.anc[(long)(r0 + s) * a.ld_anc + t] = t < L - 1 ? beam_sel(w, j) : r0 + j;
      }
    }
  }
  if (tid < W) {
    a.sum_logprob[r0 + tid] = s_nscore[tid];
    a.len[r0 + tid] = L + 1;
    if (a.src_out) a.src_out[r0 + tid] = s_src[tid];
  }
  if (tid == 0) {
    for (int e = 0; e < nf; ++e) {
      a.fin_len[(long)au * a.C + have + e] = L + 1;
      a.fin_score[(long)au * a.C + have + e] = s_fscore[e];
    }
    a.fin_n[au] = have + nf;
    a.done[au] = (have + nf >= a.C || L + 1 >= a.max_len) ? 1 : 0;
  }
}

extern "C" int wft_beam_update(const wft_beam_update_args* a, void* stream) {
  WFT_CHECK_ARG(a && a->cand_tok && a->cand_logp && a->tokens && a->anc && a->len && a->sum_logprob && a->done && a->unfinished, "null pointer");
  WFT_CHECK_ARG(a->fin_tokens && a->fin_len && a->fin_score && a->fin_n, "null pointer (finished lists)");
  WFT_CHECK_ARG(a->B >= 1 && a->W >= 1 && a->W <= BEAM_MAX_W, "beam size must lie in 1..8");
  WFT_CHECK_ARG(a->C >= 1, "the finished lists hold C >= 1 entries");
  WFT_CHECK_ARG(a->max_len >= 1 && a->max_len <= a->ld_tokens && a->max_len <= a->ld_anc, "max_len must fit the token buffer and the ancestry table");
  WFT_CHECK_ARG(a->eot >= 0, "eot outside the vocabulary");
  hipLaunchKernelGGL(beam_update_kernel, dim3((unsigned)a->B), dim3(BEAM_THREADS), 0, (hipStream_t)stream, *a);
  wft_decode_count_launch((const int*)a->done, a->B, a->unfinished, (hipStream_t)stream);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
