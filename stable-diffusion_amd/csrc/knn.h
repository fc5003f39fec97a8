// Exact k-NN search over a database of raw fp32 embeddings (knn.hip): the launches and the sdmi_knn handle's state.
#pragma once
#include "common.h"

namespace sdmi {

int knn_check_args(int64_t N, int D, int B, int k);       // the limits of the search: D % 4, D <= 1024, 1 <= B <= 64, 1 <= k <= 64, k <= N
int64_t knn_default_slab_rows(int64_t N);
// inv_norm[row] = 1 / ||db[row]||; first_bad: the first row whose inverse norm is not positive and finite, or -1 (device int64)
int launch_knn_inv_norm(const float* db, int64_t N, int D, float* inv_norm, hipStream_t s);
int launch_knn_first_bad(const float* inv_norm, int64_t N, long long* out, hipStream_t s);
// candidates [B][ceil(N / slab_rows)][k] (score, row index), unsorted; a list with fewer than k rows is padded with (-inf, INT_MAX)
int launch_knn_scan(const float* db, const float* inv_norm, int64_t N, int D, const float* queries, int B, int k, int64_t slab_rows, float* cand_s,
                    int* cand_i, hipStream_t s);
// per_group > 0: a first stage -- groups of per_group lists each reduced to k, written as [B][ceil(n_lists / per_group)][k] candidates
int launch_knn_merge(const float* cand_s, const int* cand_i, int B, int n_lists, int k, int* idx_out, float* score_out, hipStream_t s,
                     int per_group = 0);
// out[b][has_c0 + j][:] = db[idx[b][j]] * inv_norm[idx[b][j]], rows at pitch ldo floats; c0 [B][D] (or null) is copied to slot 0
int launch_knn_gather(const float* db, const float* inv_norm, int64_t N, int D, const int* idx, int B, int k, const float* c0, float* out,
                      int64_t ldo, hipStream_t s);
// a plain 16-byte read-only sweep of the buffer (the benchmark's bandwidth ceiling); sink: one float, practically never written
int launch_knn_stream_read(const float* p, int64_t n_floats, float* sink, hipStream_t s);

class Knn {
 public:
  ~Knn();
  int build(int D, int64_t capacity);
  int set_rows(int64_t first_row, int64_t n, const float* rows, hipStream_t s);
  int finalize(hipStream_t s);
  int64_t workspace_bytes(int B, int k) const;
  // scan, merge (in two stages above 64 slabs), gather.  queries fp32 [B][D] (device) -> idx [B][k], score [B][k]; nn_out [B][k][D] (or null); c0 != null: nn_out is [B][1 + k][D] with c0 in slot 0
  int search(const float* queries, int B, int k, int* idx_out, float* score_out, float* nn_out, const float* c0, void* workspace,
             int64_t ws_bytes, hipStream_t s);
  int D_ = 0;
  int64_t cap_ = 0, n_ = 0;       // n_: rows set so far (the high-water mark of set_rows)
  bool finalized_ = false;
  float* db_ = nullptr;
  float* inv_norm_ = nullptr;

 private:
  long long* first_bad_ = nullptr;
};

}  // namespace sdmi
