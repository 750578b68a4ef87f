/*
 * posecnn_train.h — C-ABI of the TRAINING side in libposecnn_hip.so: the fused
 * momentum-SGD update of a set of parameter tensors (csrc/momentum.hip).
 * A companion of posecnn_hip.h (same library, same conventions and error
 * codes); pcnn_train_abi_version() versions these entry points on their own,
 * pcnn_abi_version() does not change with them.
 *
 * Conventions (those of posecnn_hip.h)
 *  - every pointer is a DEVICE pointer unless the name ends in _host;
 *  - `stream` is a hipStream_t passed as void* (NULL = legacy default stream);
 *  - nothing allocates: temporaries live in a caller-provided `workspace` whose
 *    size the matching *_workspace_size() query returns;
 *  - nothing synchronises and nothing is read back: the op can be captured in
 *    a hipGraph, and the step counter and learning rate live on the device;
 *  - return value 0 = PCNN_OK, otherwise a PCNN_E* code (never exit()).
 */
#ifndef POSECNN_TRAIN_H
#define POSECNN_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCNN_MOMENTUM_REGULARIZE 1 /* table flags: the tensor takes the L2 term */

/* 1: pcnn_momentum_chunk, pcnn_momentum_workspace_size, pcnn_momentum_sgd */
int pcnn_train_abi_version(void);

/* ---------------------------------------------------------------------------
 * Momentum SGD: TF's ApplyMomentum (accum = accum * momentum + grad;
 * var -= lr * accum) on the gradient of loss + sum weight_reg l2_loss(var),
 * i.e. the reference's train_op MomentumOptimizer(lr, 0.9).minimize(loss) with
 * loss_regu in the loss (lib/fcn/train.py:481,530-534; network.py:417-419
 * regularises the fc weights and biases), for every tensor of a set in one
 * launch, in place, followed by a one-block finishing kernel on the same
 * stream (two launches per call).
 *
 *  table (T,5) int64, one row per tensor:
 *    [0] address of the parameter w (n) f32, read and written
 *    [1] address of the gradient g (n) f32, read only
 *    [2] address of the momentum accumulator m (n) f32, read and written
 *    [3] n, the element count (0 is fine: the tensor has no chunk)
 *    [4] flags: PCNN_MOMENTUM_REGULARIZE
 *  chunk_start (T+1) int32: the prefix sum of ceil(n / pcnn_momentum_chunk())
 *    over the tensors; chunk_start[T] = total_chunks.  The unit of work is a
 *    chunk of pcnn_momentum_chunk() consecutive elements of ONE tensor (the
 *    last chunk of a tensor may be short; chunks never straddle tensors).
 *  The addresses are packed (contiguous) arrays, 4-byte aligned.  A tensor
 *  whose three addresses are all 16-byte aligned moves 16 bytes per lane on
 *  all five streams; a tensor with any address only 4-byte aligned (a view at
 *  an odd element offset) takes a scalar path as a whole; a tail of fewer
 *  than 4 elements is scalar.  Both paths compute the same bits.  The 3 T
 *  arrays of one call must not overlap.  The library cannot check the table:
 *  a wrong address, count or chunk_start is a stray device access.
 *
 * Arithmetic: float32, every operation rounded separately (no FMA).  Per
 * element of a tensor with the flag set
 *      t  = weight_reg * w
 *      g2 = g + t                 (flag clear: g2 = g)
 *      a  = momentum * m
 *      m' = a + g2
 *      u  = lr * m'
 *      w' = w - u
 *
 * Learning rate: exponential_decay(lr0, global_step, stepsize, gamma,
 * staircase=True) read before global_step is incremented.  step_dev (1) int64
 * holds the number of updates applied so far, n; with p = stepsize > 0 ?
 * n / stepsize : 0, lr = (float)(lr0 gamma^p), the power taken in float64 by
 * p multiplications (double)lr0 * (double)gamma * (double)gamma ..., left to
 * right (not pow()).  The update only reads the counter; the finishing kernel,
 * behind every block of the update in stream order, stores n + 1 and, if
 * lr_out (1) f32 is not NULL, the lr this call used.
 *
 * Regularisation loss (reg_loss (1) f32; NULL: not computed, `workspace` is
 * not touched): weight_reg / 2 times the sum of w^2 over the flagged tensors,
 * on the weights BEFORE the update (those the forward pass used).
 * Deterministic, no atomics; with c = pcnn_momentum_chunk() = 4096 and blocks
 * of 256 threads:
 *  - thread t of a chunk owns the elements 4 (t + 256 j) + k, j = 0..3,
 *    k = 0..3, and adds their squares to 0 in that order (j outer) in f32;
 *  - the 64 lanes of a wave add as a butterfly, v += v[lane ^ o] for o = 32,
 *    16, 8, 4, 2, 1; the four waves' sums as (s0 + s1) + (s2 + s3): one f32
 *    partial per chunk in workspace[chunk] (0 for a chunk of an unflagged
 *    tensor);
 *  - the finishing kernel (1024 threads) adds the partials in float64: thread
 *    t the chunks t, t + 1024, ... in ascending order, the 64 lanes of a wave
 *    as the same butterfly, the 16 waves' sums in ascending order; then
 *    reg_loss[0] = (float)(((double)weight_reg * 0.5) * sum), rounded once.
 *    (One thread adding every partial in ascending order would put a serial
 *    chain of total_chunks dependent float64 additions behind each update.)
 *  Two runs on the same data give the same bits.
 *
 * workspace: pcnn_momentum_workspace_size(total_chunks) bytes, needed only
 * with reg_loss.
 * T = 0 is fine: the call only counts the step (and writes reg_loss = 0).
 * The launches do not consume a completion event armed by
 * pcnn_set_completion_event for another op.
 * PCNN_EINVAL: a NULL table or chunk_start with T > 0, a NULL step_dev, T < 0,
 * total_chunks outside [0, 2^31), momentum outside [0, 1), lr0 < 0,
 * weight_reg < 0, gamma <= 0, stepsize < 0 (or any of them NaN), reg_loss
 * with a NULL or too small workspace.
 * ------------------------------------------------------------------------- */
int pcnn_momentum_chunk(void);
size_t pcnn_momentum_workspace_size(long total_chunks);
int pcnn_momentum_sgd(const int64_t* table, const int32_t* chunk_start, int T, long total_chunks, float lr0,
                      float gamma, int stepsize, float momentum, float weight_reg, int64_t* step_dev,
                      float* reg_loss, float* lr_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_TRAIN_H */
