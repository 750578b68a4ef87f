/*
 * posecnn_image.h — C-ABI of the network's INPUT side in libposecnn_hip.so: the
 * lit colour rendering of synthetic scenes and the picture -> input-blob pass.
 * A companion of posecnn_hip.h (same library, same conventions, error codes
 * and pcnn_abi_version, which is >= 8 when these entry points exist).
 *
 * Conventions (those of posecnn_hip.h)
 *  - every pointer is a DEVICE pointer unless the name ends in _host;
 *  - `stream` is a hipStream_t passed as void* (NULL = legacy default stream);
 *  - nothing allocates: temporaries live in a caller-provided `workspace` whose
 *    size the matching *_workspace_size() query returns;
 *  - nothing synchronises and nothing is read back: both ops can be captured
 *    in a hipGraph;
 *  - return value 0 = PCNN_OK, otherwise a PCNN_E* code (never exit()).
 */
#ifndef POSECNN_IMAGE_H
#define POSECNN_IMAGE_H

#include <stddef.h>
#include <stdint.h>

#include "posecnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PCNN_IMAGE_CHROMATIC 1 /* flags: apply the HLS jitter (step 3) */
#define PCNN_IMAGE_NOISE 2     /* flags: add the Gaussian noise (step 4) */
#define PCNN_IMAGE_NCHW 4      /* flags: blob (B,3,H,W) instead of (B,H,W,3) */

/* ---------------------------------------------------------------------------
 * Lit scene renderer: pcnn_render_scenes with a colour attachment, i.e. the
 * Phong-lit colour pass Synthesizer::render draws next to the vertex map
 * (synthesize.cpp:473-536, 575-590 with lib/kinect_fusion/shaders/
 * canonicalVertsAndColor.vert / .frag): one light per scene, one shininess per
 * instance, specular colour 1 (glRender.h:246).
 *  Every argument of pcnn_render_scenes, with its meaning, checks and outputs:
 *    the seven maps are written by the same passes and the same expressions and
 *    carry pcnn_render_scenes's bits.  In addition:
 *  colors (V_total,3) f32 RGB in [0, 1] per vertex, packed like `vertices`
 *  shininess (K) f32 the specular exponent of each instance
 *  lights (S,8) f32 per scene [x y z w, intensity, attenuation, ambient, 0]:
 *    the position in the CAMERA frame; w = 0 a directional light (x y z its
 *    direction towards the light, no attenuation)
 *  color (S,H,W,4) f32 BGRA (the reference downloads GL_BGRA), 16-byte aligned,
 *    every element written: (0, 0, 0, 0) off the models, and on them, with
 *    the winner's perspective-correct weights la, lb, lc (those of the other
 *    maps) and its three vertices a, b, c,
 *      P = (la Pa + lb Pb) + lc Pc   camera-frame position (pred_vertices of
 *                                    pcnn_render_meshes)
 *      N = (la Na + lb Nb) + lc Nc   the rotated unit vertex normals, then
 *                                    N / |N| (a zero length is left as is)
 *      c = (la ca + lb cb) + lc cc   the vertex colours
 *      D = light.xyz - P, att = 1 / (1 + attenuation |D|^2)
 *          (w = 0: D = light.xyz, att = 1)
 *      L = D / |D|, V = -P / |P|, nl = N.L, diffuse = max(0, nl)
 *      specular = diffuse > 0 ? pow(max(0, V.(2 nl N - L)), shininess) : 0
 *      rgb = (ambient c) I + att ((diffuse c) I + specular I), alpha = 1
 *    in float32, every operation rounded separately, dot products and squared
 *    lengths summed as (x + y) + z, one 16-byte store (b, g, r, 1) per pixel.
 *    The value is linear and unclamped (it may exceed 1); pcnn_image_blob
 *    quantises it.
 *  Narrowings: the reference interpolates the raw model normal and normalises
 *    after rotating, here the per-vertex rotated normals are already of unit
 *    length -- the two agree for unit mesh normals; there is no texture path
 *    (canonicalVertsAndTexture.*): the surface colour is the interpolated
 *    vertex colour.
 *  workspace: pcnn_render_scenes_lit_workspace_size (16-byte aligned).
 *  PCNN_EINVAL / PCNN_ECAPACITY: as pcnn_render_scenes, plus a NULL or
 *  misaligned new argument.
 * ------------------------------------------------------------------------- */
size_t pcnn_render_scenes_lit_workspace_size(int S, int K, int H, int W, int V_total, int F_max);
int pcnn_render_scenes_lit(const float* vertices, const float* normals, const float* colors, const int32_t* faces,
                           const int32_t* vert_offset, const int32_t* face_offset, int M, int V_total, int F_total,
                           int F_max, const int32_t* mesh_index, const int32_t* class_id, const float* poses,
                           const float* shininess, int K, const int32_t* scene_offset, const float* lights, int S,
                           int H, int W, float fx, float fy, float px, float py, float znear, float zfar,
                           int32_t* label, float* depth, float* vertmap, float* vertex3, int32_t* inst_id,
                           int32_t* visible, float* centers, float* color, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---------------------------------------------------------------------------
 * Image blob: a rendered picture into the network's input in one pass, i.e.
 * _get_image_blob (gt_synthesize_layer/minibatch.py:132-187) with
 * chromatic_transform and add_noise (lib/utils/blob.py:74-129).
 *  color (B,H,W,4) f32 BGRA as pcnn_render_scenes_lit writes it, 16-byte aligned
 *  backgrounds (N_bg,H,W,3) uint8 BGR (may be NULL when N_bg = 0)
 *  bg_index (B) int32 the background of each image; outside [0, N_bg): black
 *  jitter (B,4) f32 per image [d_h, d_l, d_s, sigma], 16-byte aligned
 *  pixel_means (3) f32 in BGR order (PIXEL_MEANS, lib/fcn/config.py:242)
 *  seed, image_offset: the noise of image b depends on (seed, image_offset + b,
 *    pixel) alone, so a shard reproduces the frames of a single-device run
 *  flags: PCNN_IMAGE_CHROMATIC | PCNN_IMAGE_NOISE | PCNN_IMAGE_NCHW
 *  blob (B,H,W,3) f32, or (B,3,H,W) with PCNN_IMAGE_NCHW; 16-byte aligned,
 *    every element written
 * Per pixel and channel, in the reference's order:
 *  1 u8 = (uint8)min(max(255 c, 0), 255), truncated (train_net.py:200-201; a
 *    NaN gives 0)
 *  2 alpha == 0: the background's pixel instead, or 0 (minibatch.py:150-156)
 *  3 chromatic (blob.py:86-94): BGR -> HLS by the hexcone formula in f32 on
 *    u8 / 255 (l = (max + min) / 2, s = d / (max + min) below l = 0.5 else
 *    d / ((2 - max) - min), h = 60 (x - y) / d + {0, 120, 240}, + 360 when
 *    negative), stored 8-bit as H = rint(h / 2) with 180 -> 0, L = rint(255 l),
 *    S = rint(255 s); H + d_h modulo 180, L + d_l and S + d_s clipped to
 *    [0, 255], all three truncated; HLS -> BGR (p2 = l (1 + s) up to l = 0.5
 *    else (l + s) - l s, p1 = 2 l - p2, the six sectors of H / 30) ending in
 *    rint(255 x) saturated.  This is the standard formula, not OpenCV's 8-bit
 *    code path, whose own rounding is not pinned.
 *  4 noise (blob.py:108-116): v + sigma z clipped to [0, 255], one normal
 *    deviate z per pixel shared by the channels: Box-Muller
 *    sqrt(-2 log u1) cos(2 pi u2) in double, rounded to f32 once, from the
 *    Philox4x32-10 block of counter (pixel, 0, lo, hi of image_offset + b)
 *    under key (seed lo ^ 0x494D4731, seed hi); u1 = (word 0 + 1) / 2^32 in
 *    (0, 1], u2 = word 1 / 2^32
 *  5 (float)v - pixel_means[channel] (minibatch.py:182-183)
 * Not done here: add_noise's 10 % motion-blur branch, background resizing
 * (backgrounds arrive at H x W), flipping and multi-scale, the DEPTH, RGBD
 * and NORMAL inputs.
 * PCNN_EINVAL: a NULL required pointer, B, H or W <= 0, N_bg < 0, H W >= 2^31,
 * unknown flags, misalignment.
 * ------------------------------------------------------------------------- */
int pcnn_image_blob(const float* color, const uint8_t* backgrounds, int N_bg, const int32_t* bg_index,
                    const float* jitter, const float* pixel_means, uint64_t seed, int64_t image_offset, int B, int H,
                    int W, int flags, float* blob, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* POSECNN_IMAGE_H */
