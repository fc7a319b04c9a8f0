// What the inference files share across translation units (host side, namespace cc), included by the
// callers and by the defining file alike, so that a changed signature fails to compile.
#pragma once
#include "common.hpp"

namespace cc {
// api.cpp: the flat parameter layout
int param_offsets(int V, int d, int64_t *off, int64_t *size, int64_t *total, int64_t *main_total);

// infer.hip
int infer_check_d(int d, const char *who);
int infer_gather_cap(int max_n);
int infer_h3_launch(const float *params, int V, int d, int R, const int32_t *row_ptr,
                    const int32_t *idx, int max_n, float *part, float *zlat, float *h3,
                    hipStream_t s);
int infer_towers_launch(const float *params, int V, int d, int R, const int32_t *one_ptr,
                        const float *e1, float *zlat, float *h3, hipStream_t s);

// recbatch.hip
int row_bits_launch(const int32_t *row_ptr, const int32_t *idx, int R, int V, int VW, uint32_t *bits,
                    hipStream_t s);
int pools_check(const char *who, const uint32_t *pools, int n_pools, const int32_t *pool_of_row,
                bool optional);
int batch_max_amount();
size_t batch_select_ws_bytes(int V, int d, int R, int max_n, bool pooled);
int batch_select_launch(const float *params, int V, int d, int R, const int32_t *row_ptr,
                        const int32_t *idx, int max_n, int amount, void *ws, int32_t *n_add,
                        int32_t *additions, float *add_vals, float *cut_vals, float *probs,
                        const uint32_t *pools, int n_pools, const int32_t *pool_of_row,
                        hipStream_t s);
}  // namespace cc
