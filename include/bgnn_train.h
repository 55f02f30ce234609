/*
 * bgnn_train.h -- C ABI of libbgnn_hip.so, training part: the backward pass of BathymetricGNN (ABI 7).
 *
 * The conventions of bgnn.h hold (DEVICE / HOST pointers, return codes, bgnn_last_error(), the context's stream); this header
 * adds the entry points that let the reference's training loop (training/trainer.py:732-761: model.train(), outputs =
 * model(batch), losses['total'].backward(), clip_grad_norm_, optimizer.step()) run on the library.  The Python mirror binds them
 * in bathymetric_gnn_amd/runtime.py (_TRAIN_SIGNATURES).
 */
#ifndef BGNN_TRAIN_H
#define BGNN_TRAIN_H

#include "bgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- backward pass (ABI 7): training BathymetricGNN (the reference's training/trainer.py:732-761 loop) ------------------------
 * A taped training forward saves the activations the backward needs in a caller-owned DEVICE buffer (the tape); bgnn_backward
 * turns the gradients of the outputs into the gradient of every weight.  Covered: the GAT backbone, hidden 32 / 64 / 128,
 * power-of-two heads with heads * hidden <= 256, any layer count, 1..4 edge features, stencil and foreign (bgnn_graph_from_edges)
 * graphs; the GraphSAGE and GIN backbones, hidden 32 / 64 / 128, any layer count, every graph their training forward accepts
 * (stencil graphs, foreign graphs without explicit self loops); exact float32.  Anything else (GCN, zero-padded shapes, wider GAT
 * layers) -> BGNN_ERR_UNSUPPORTED with a message naming the limit.  All sums are deterministic (no float atomics): two backward
 * calls on one tape give bit-identical gradients.
 *
 * bgnn_tape_bytes: bytes of the tape for this model and graph (0 and bgnn_last_error() set when the model has no backward pass).
 *   Per node (rows of the graph), GAT: 4 * (2 hid + sum over layers of (heads_l hid + 2 heads_l + 2 width_l) + head units) bytes,
 *   plus 16 bytes per channel of statistics -- 11 KB per node for the default shape (hidden 64, heads 4, 4 layers, edge_dim 3),
 *   about 11.5 GB for 16 tiles of 256 x 256.  GraphSAGE / GIN: 4 * (2 hid + layers * k hid + head units) bytes, k = 3 (SAGE: mean,
 *   z, output) or 4 (GIN: s, u, z, output) -- 3.9 / 4.9 KB per node at hidden 64, 4 layers (counts of the tables, not measurements).
 * bgnn_forward_train_tape: bgnn_forward_train_dropout (same outputs and statistics, bit for bit) that also copies its activations
 *   into `tape` (tape_bytes >= bgnn_tape_bytes).  The tape stays valid until the caller frees it; several tapes may be live.
 * bgnn_backward: reads the tape of the same model and graph (neither changed since) and the output gradients `gin` (DEVICE, each
 *   may be NULL = zero): d class_logits [N, classes], d class_probs [N, classes] (taken through the softmax), d confidence [N]
 *   (through the sigmoid), d correction [N].  Writes grad_weights (DEVICE float32 [bgnn_model_weight_count]) in the order
 *   bgnn_model_create documents; the running_mean / running_var slots are 0.  Overwrites, does not accumulate.  Asynchronous. */
size_t bgnn_tape_bytes(const bgnn_model *model, const bgnn_graph *graph);
int bgnn_forward_train_tape(bgnn_ctx *ctx, bgnn_model *model, bgnn_graph *graph, const bgnn_dropout *dropout, float *bn_batch_mean,
                            float *bn_batch_var, const bgnn_outputs *out, void *tape, size_t tape_bytes);
typedef struct bgnn_output_grads { /* all DEVICE, any may be NULL */
  const float *class_logits;  /* [N, classes] */
  const float *class_probs;   /* [N, classes] */
  const float *confidence;    /* [N]          */
  const float *correction;    /* [N]          */
} bgnn_output_grads;
int bgnn_backward(bgnn_ctx *ctx, bgnn_model *model, bgnn_graph *graph, const void *tape, const bgnn_output_grads *gin,
                  float *grad_weights);

#ifdef __cplusplus
}
#endif
#endif /* BGNN_TRAIN_H */
