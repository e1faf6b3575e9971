// edit.hip — Levenshtein alignment counts (hits, substitutions, deletions, insertions) of a ragged batch of symbol pairs, ONE launch
// (include/wft.h "Edit counts" is the contract; the evaluator's WER / CER).
//
// wft_edit_counts_i32: one workgroup per pair, sweeping the anti-diagonals d = 0 .. n + m of the (n + 1) x (m + 1) table.  A cell is one
// 64-bit word, cost << 48 | S << 32 | D << 16 | I (every field <= 4096 < 2^16), so a candidate is one 64-bit add and the comparison reads
// the top field only.  Three rotating diagonals live in LDS, ALWAYS indexed by the reference position i: cell (i, d - i) of diagonal d sits
// at index i, its predecessors at index i - 1 of diagonal d - 2 (diagonal), i - 1 of d - 1 (deletion) and i of d - 1 (insertion).  Indexing
// by the reference whatever the lengths means the problem is never transposed, so deletions, insertions and their tie priority keep their
// roles; the price is that a diagonal buffer holds max_len + 1 cells even when the hypothesis is the shorter side.  Diagonal d is written
// while d - 1 and d - 2 are read and the buffer of d - 3 is the one overwritten, so ONE barrier per diagonal orders everything.  Both
// symbol rows are staged in LDS once (r is then read ascending, h descending along a diagonal).  Dynamic LDS is sized from max_len:
// 3 (max_len + 1) 8 + 2 max_len 4 bytes, 131 096 at the cap and 19 KiB at 605 symbols, where eight workgroups share a CU.
// The table is device memory, so the row check is the kernel's own and uniform over the workgroup; a failed row reads no symbol.
// A side kernel of the evaluator: plain C++, integers only, no atomics.
#include "gemm_common.h"  // DynLdsOnce: the cap needs more than the 64 KiB a kernel may ask for by default

#define EDIT_THREADS 256
#define EDIT_MAX_LEN 4096
#define EDIT_MAX_P (1 << 20)

typedef unsigned long long edit_cell;
#define EDIT_COST (1ull << 48)
#define EDIT_S (EDIT_COST | (1ull << 32))
#define EDIT_D (EDIT_COST | (1ull << 16))
#define EDIT_I (EDIT_COST | 1ull)

static inline int edit_lds_bytes(int max_len) { return 3 * (max_len + 1) * (int)sizeof(edit_cell) + 2 * max_len * (int)sizeof(int); }

__global__ __launch_bounds__(EDIT_THREADS) void edit_counts_kernel(const int* sym, long long n_sym, const wft_edit_row* rows, int* out,
                                                                   long long ld_out, int max_len) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const wft_edit_row r = rows[blockIdx.x];
  int* o = out + (long long)blockIdx.x * ld_out;
  const int n = r.ref_len, m = r.hyp_len;
  // the check: uniform over the workgroup (n_sym - n cannot overflow: 0 <= n <= max_len once the first clause holds)
  const bool ok = n >= 0 && n <= max_len && m >= 0 && m <= max_len && r.ref_off >= 0 && r.hyp_off >= 0 && r.ref_off <= n_sym - n &&
                  r.hyp_off <= n_sym - m;
  if (!ok) {
    if (tid < 4) o[tid] = -1;
    return;
  }
  const int stride = max_len + 1;
  edit_cell* cur = reinterpret_cast<edit_cell*>(smem);  // diagonal d
  edit_cell* p1 = cur + stride;                          // diagonal d - 1
  edit_cell* p2 = p1 + stride;                           // diagonal d - 2
  int* rs = reinterpret_cast<int*>(p2 + stride);
  int* hs = rs + max_len;
  const int* rg = sym + r.ref_off;
  const int* hg = sym + r.hyp_off;
  for (int k = tid; k < n; k += EDIT_THREADS) rs[k] = rg[k];
  for (int k = tid; k < m; k += EDIT_THREADS) hs[k] = hg[k];
  __syncthreads();
#pragma unroll 1
  for (int d = 0; d <= n + m; ++d) {
    const int lo = max(0, d - m), hi = min(n, d);
    for (int i = lo + tid; i <= hi; i += EDIT_THREADS) {
      const int j = d - i;
      edit_cell best;
      if (i == 0) {
        best = (edit_cell)j * EDIT_I;
      } else if (j == 0) {
        best = (edit_cell)i * EDIT_D;
      } else {
        best = p2[i - 1] + (rs[i - 1] != hs[j - 1] ? EDIT_S : 0ull);
        const edit_cell del = p1[i - 1] + EDIT_D, ins = p1[i] + EDIT_I;
        if ((del >> 48) < (best >> 48)) best = del;  // a later candidate wins only when strictly cheaper
        if ((ins >> 48) < (best >> 48)) best = ins;
      }
      cur[i] = best;
    }
    __syncthreads();
    edit_cell* t = p2;  // the buffer of d - 2 is free once every thread has passed the barrier: it becomes diagonal d + 1
    p2 = p1;
    p1 = cur;
    cur = t;
  }
  if (tid == 0) {
    const edit_cell v = p1[n];  // cell (n, m) of the last diagonal
    const int S = (int)((v >> 32) & 0xffffu), D = (int)((v >> 16) & 0xffffu), I = (int)(v & 0xffffu);
    o[0] = n - S - D;
    o[1] = S;
    o[2] = D;
    o[3] = I;
  }
}

extern "C" int wft_edit_max_len(void) { return EDIT_MAX_LEN; }
extern "C" int wft_edit_threads(void) { return EDIT_THREADS; }

extern "C" int wft_edit_counts_i32(const int32_t* sym, int64_t n_sym, const wft_edit_row* rows, int32_t* out, int64_t ld_out, int P,
                                   int max_len, void* stream) {
  WFT_CHECK_ARG(sym && rows && out, "null pointer");
  WFT_CHECK_ARG(n_sym >= 1, "n_sym must be at least 1");
  WFT_CHECK_ARG(P >= 1 && P <= EDIT_MAX_P && max_len >= 1 && max_len <= EDIT_MAX_LEN, "bad shape (1 <= P <= 2^20, 1 <= max_len <= 4096)");
  WFT_CHECK_ARG(ld_out >= 4, "leading dimension smaller than the four counts");
  WFT_CHECK_ARG((uintptr_t)sym % 4 == 0 && (uintptr_t)rows % 8 == 0 && (uintptr_t)out % 4 == 0, "rows must be 8-byte, sym and out 4-byte aligned");
  static_assert(sizeof(wft_edit_row) == 32, "wft_edit_row is 32 bytes");
  static_assert(3 * (EDIT_MAX_LEN + 1) * 8 + 2 * EDIT_MAX_LEN * 4 <= 160 * 1024, "the cap fits one CU's LDS");
  static DynLdsOnce once;  // raised once per device to what the cap needs; a launch asks for what its max_len needs
  if (!once.set(edit_counts_kernel, edit_lds_bytes(EDIT_MAX_LEN))) return WFT_ERR_LAUNCH;
  hipLaunchKernelGGL(edit_counts_kernel, dim3((unsigned)P), dim3(EDIT_THREADS), edit_lds_bytes(max_len), (hipStream_t)stream, sym,
                     (long long)n_sym, rows, out, (long long)ld_out, max_len);
  WFT_CHECK_LAUNCH();
  return WFT_OK;
}
