/*
 * bgnn_optim.h -- C ABI of libbgnn_hip.so, optimizer part: the last two lines of the reference's training loop
 * (training/trainer.py:759-761: clip_grad_norm_, optimizer.step()) on the weight blob, and the packed model brought up to date
 * where it lies (ABI 7; no entry point of bgnn.h / bgnn_train.h changes).
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream, asynchronous).
 * The Python mirror binds these in bathymetric_gnn_amd/runtime.py (_OPTIM_SIGNATURES); training/optim.py (FusedAdamW) drives them.
 */
#ifndef BGNN_OPTIM_H
#define BGNN_OPTIM_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One updated slot of the blob: `count` floats at `offset` (bgnn_model_weight_count order; one slot per parameter tensor), and
 * the number of steps this slot has taken INCLUDING this one (>= 1; its bias corrections are 1 - beta^step). */
typedef struct bgnn_adamw_slot {
  uint64_t offset;
  uint64_t count;
  int64_t step;
} bgnn_adamw_slot;

typedef struct bgnn_adamw_params {
  double lr, beta1, beta2, eps, weight_decay;
  double max_norm; /* gradient clipping: <= 0 or +inf = none */
} bgnn_adamw_params;

#define BGNN_ADAMW_CHUNK 2048 /* elements behind one partial sum of squares (fixed: the summation order is part of the result) */

/* bgnn_adamw_step: torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.AdamW.step() (decoupled weight decay,
 *   bias correction per slot, no amsgrad, no maximize) over flat DEVICE float32 blobs of n_weights floats each: the master weights,
 *   the gradient (bgnn_backward's layout), exp_avg and exp_avg_sq.  `slots` (HOST, n_slots entries, disjoint, inside the blob) lists
 *   what is updated; everything else -- BatchNorm running statistics, the zero edge weights of an edge_dim=None model, a parameter
 *   without a gradient this step -- is neither read nor written, in any of the four blobs.
 *   total_norm = sqrt(sum over the listed slots of g^2) is written to grad_norm (DEVICE float, may be NULL): what clip_grad_norm_
 *   returns.  With clipping, every gradient is multiplied by min(1, max_norm / (total_norm + 1e-6)) first (the gradient blob itself
 *   is left as it is).
 *   Arithmetic: per element in float64 from the float32 inputs, weights and both moments rounded to float32 once per step.  The
 *   sum of squares is float64 in a fixed order -- one partial per BGNN_ADAMW_CHUNK elements of a slot, each by a fixed tree, then
 *   a fixed-order sum of the partials; no atomics: equal inputs give equal bits.  Non-finite gradients propagate as in torch (an
 *   inf / NaN norm makes every clipped gradient NaN / 0 the same way).
 *   Three launches and one small table upload; no allocation in the steady state; the host does not wait. */
int bgnn_adamw_step(bgnn_ctx *ctx, float *weights, const float *grads, float *exp_avg, float *exp_avg_sq, size_t n_weights,
                    const bgnn_adamw_slot *slots, int32_t n_slots, const bgnn_adamw_params *params, float *grad_norm);

#define BGNN_REFRESH_ALL 0   /* every weight may have changed */
#define BGNN_REFRESH_STATS 1 /* only BatchNorm running statistics changed since the last create / refresh */

/* bgnn_model_refresh_prepare: builds the model's gather tables (one device allocation, made by running the host packer of
 *   bgnn_model_create over an index-valued blob); idempotent.  bgnn_model_refresh calls it on first use; call it yourself to keep
 *   that one allocation out of the training loop.
 * bgnn_model_refresh: brings a live model up to date from `weights` (DEVICE float32 [n_weights], bgnn_model_weight_count order),
 *   in place: no allocation (after the tables exist), no free, the host does not wait.  Rewritten: everything the training
 *   forwards and bgnn_backward read -- the blob as given, the extractor's and the layers' transposed weights and biases, attention
 *   vectors, the folded edge vectors V, unfolded BatchNorm weights, the heads' tables, the extractor's second Linear folded into
 *   lin of layer 0 and its re-layouts.  V and the fold are float64 dot products in the host packer's own order: the float32
 *   values are those bgnn_model_create would have packed.
 *   What only the eval forward reads -- BatchNorm folded into scale / shift, the operand-split / bf16 / tile-group images, the
 *   fused heads' table, the cached tables of V over the canonical edge attributes -- is marked stale instead: the next
 *   bgnn_forward / bgnn_feature_extractor / bgnn_heads / bgnn_infer_tiles on the model completes it first (one download of the
 *   blob, the host packer, one upload into the same allocation; that call waits for the stream).  A model that was never
 *   refreshed is never stale.
 *   `what` = BGNN_REFRESH_STATS: the caller vouches that only running statistics differ from the last refresh; the blob copy is
 *   taken and the eval images marked stale, nothing else runs.
 *   A zero-padded model (hidden / heads outside the kernels' widths) -> BGNN_ERR_UNSUPPORTED: it cannot train either. */
int bgnn_model_refresh_prepare(bgnn_ctx *ctx, bgnn_model *model);
int bgnn_model_refresh(bgnn_ctx *ctx, bgnn_model *model, const float *weights, size_t n_weights, int32_t what);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_OPTIM_H */
