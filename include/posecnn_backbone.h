/*
 * posecnn_backbone.h — C-ABI of the VGG16 BACKBONE's forward layers in
 * libposecnn_hip.so: 3x3 convolution + bias + ReLU and 2x2 max-pool
 * (csrc/backbone.hip), the layers of lib/networks/vgg16_convs.py:80-97 that
 * turn the (B,H,W,3) blob into conv4_3 and conv5_3.  A companion of
 * posecnn_hip.h (same library, same conventions and error codes);
 * pcnn_backbone_abi_version() versions these entry points on their own,
 * pcnn_abi_version() does not change with them.
 *
 * Conventions (those of posecnn_hip.h)
 *  - every pointer is a DEVICE pointer unless the name ends in _host;
 *  - `stream` is a hipStream_t passed as void* (NULL = legacy default stream);
 *  - nothing allocates: temporaries live in a caller-provided `workspace` whose
 *    size the matching *_workspace_size() query returns;
 *  - nothing synchronises and nothing is read back: every op can be captured in
 *    a hipGraph;
 *  - return value 0 = PCNN_OK, otherwise a PCNN_E* code (never exit()).
 *
 * Layouts: maps are NHWC float32, contiguous.  Weights are the reference's TF
 * variables as they are: HWIO (3,3,Cin,Cout), i.e. a row-major (9 Cin, Cout)
 * matrix with row k = (dy 3 + dx) Cin + c; bias (Cout).  Padding is TF SAME at
 * stride 1: a one-pixel border of zeros.
 */
#ifndef POSECNN_BACKBONE_H
#define POSECNN_BACKBONE_H

#include <stddef.h>
#include <stdint.h>

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: pcnn_conv3x3_workspace_size, pcnn_conv3x3_fwd, pcnn_maxpool2x2_fwd */
int pcnn_backbone_abi_version(void);

/* ---------------------------------------------------------------------------
 * y (B,H,W,Cout) = act(conv3x3(x (B,H,W,Cin), weights) + bias), stride 1, SAME.
 * act: 0 none, 1 ReLU (v > 0 ? v : 0).  bias may be NULL (no bias is added).
 * precision: 2 only (the exact three-way bf16 split of pcnn_gemm's precision 2);
 * the parameter is there so that other precisions can follow without an ABI
 * break.
 *
 * Arithmetic
 *  - Cin % 16 == 0: an implicit GEMM on v_mfma_f32_32x32x16_bf16 with both
 *    operands split exactly into three bf16 planes and the six plane products
 *    of posecnn_hip.h's precision 2 kept: each of the 9 Cin products within
 *    2^-24 |x||w| of exact, float32 accumulation in an unspecified but fixed
 *    order, then bias, then ReLU; deterministic (two calls give the same bits;
 *    no float atomics).  Taps outside the image contribute exact zeros.
 *    Operand range, as precision 2 of pcnn_gemm: finite |x| <= 3.3895314e38
 *    (the largest bf16); there results track fp32.  An inf / NaN operand, or a
 *    finite one above that bound (its hi plane rounds to inf), makes the output
 *    elements it reaches NaN (fp32 would give +-inf or a finite value); every
 *    other element is unaffected.
 *  - Cin == 3 (conv1_1): direct float32, in a fixed order.  Per output: s = 0;
 *    for dy = 0..2, dx = 0..2, c = 0..2 in that nesting, s = s + x * w with the
 *    product and the sum rounded separately (no FMA); taps outside the image
 *    are skipped; then v = s + bias, then v > 0 ? v : 0.
 *
 * Small maps may split the contraction over slices whose partial sums go to
 * `workspace` and are added in slice order by a second launch; the split is a
 * function of (B, H, W, Cin, Cout) alone.  pcnn_conv3x3_workspace_size returns
 * the bytes that needs: 0 for shapes pcnn_conv3x3_fwd refuses, and 0 for shapes
 * that need none (workspace may then be NULL).  One or two launches.
 *
 * PCNN_EINVAL: precision != 2; act not 0 or 1; a dimension < 1; Cin neither 3
 * nor a multiple of 16; Cout % 4 != 0; an input or output map, or the weights,
 * of 2^31 bytes or more (the buffer views address with 32-bit offsets); a NULL
 * or not 16-byte aligned x, weights or y; a misaligned bias; x == y; a NULL or
 * misaligned workspace where one is needed.
 * PCNN_ECAPACITY: workspace_bytes below pcnn_conv3x3_workspace_size(...).
 * ------------------------------------------------------------------------- */
size_t pcnn_conv3x3_workspace_size(int B, int H, int W, int Cin, int Cout, int precision);
int pcnn_conv3x3_fwd(const float* x, const float* weights, const float* bias, int B, int H, int W, int Cin, int Cout,
                     int act, int precision, float* y, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * y (B, ceil(H/2), ceil(W/2), C) = 2x2 max-pool of x (B,H,W,C), stride 2, TF
 * SAME: window (oy, ox) holds rows 2 oy, 2 oy + 1 and columns 2 ox, 2 ox + 1,
 * those inside the map -- the last window of an odd axis holds one row or
 * column, and padding never wins.  Per output: m = x[2 oy][2 ox], then
 * m = v > m ? v : m over the present ones of (0,1), (1,0), (1,1) in that order.
 * C % 4 == 0.  One launch.
 *
 * PCNN_EINVAL: a dimension < 1, C % 4 != 0, a map of 2^31 bytes or more, a NULL
 * or not 16-byte aligned x or y, x == y.
 * ------------------------------------------------------------------------- */
int pcnn_maxpool2x2_fwd(const float* x, int B, int H, int W, int C, float* y, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_BACKBONE_H */
