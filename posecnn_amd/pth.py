"""The PyTorch module API the reference's my_tools scripts call
(my_tools/convert_to_pth.py:104-178, my_tools/loss_pth.py:51-64), backed by
the HIP ops of this package.  The reference imports these from a `lib/model`
package that it does not ship; the signatures here follow
its call sites:

    HoughVoting(num_classes, threshold_vote, threshold_percentage,
                label_threshold=500, inlier_threshold=0.9, skip_pixels=1,
                is_train=False)(label_2d, vertex_pred_NHWC, extents, poses, meta_data)
        -> (top_box, top_pose, top_target, top_weight, top_domain)
    _RoIPooling(pooled_height, pooled_width, spatial_scale)(features_NCHW, rois_Nx5)
        -> pooled (N, C, PH, PW)          rois: [batch, x1, y1, x2, y2]
    AverageDistanceLoss(num_classes, margin)(pred, target, weight, points, symmetry)
        -> loss (1,)

The two dense-map terms of the objective (lib/fcn/train.py:489-515), which the
reference builds from TF ops, as modules over posecnn_amd.losses:

    SegmentationLoss(threshold)(score_NHWC, gt_label_2d) -> (loss, label_2d)
    VertexLoss(sigma=1.0, w_inside=10.0)(vertex_pred, vertex_targets, vertex_weights) -> loss
                                        (vertex_pred, label, vertex3)                 -> loss

and the class-compact vertex_pred layer (posecnn_amd.vertex_pred) as a
trainable module:

    VertexPredCompact(num_units, num_classes)(feat_NHWC, label) -> (B,H,W,3)

The upscore layers in front of both heads (posecnn_amd.upscore), and the two
heads with the upscore folded behind their 1x1 conv (x_low is the feature map
at 1/stride resolution, the (B,H,W,num_units) map between the layers is never
formed; equal to the reference's order in exact arithmetic, different from it
by float32 rounding):

    Upscore(stride, relu=False)(x_NHWC) -> (B, stride*h, stride*w, Ch)
    VertexHeadCompact(num_units, num_classes, stride=8)(x_low, label) -> (B,H,W,3)
    ScoreHead(num_units, num_classes, stride=8)(x_low) -> score (B,H,W,C)

and the layer group in front of both heads (posecnn_amd.neck: the four 1x1
convs on conv4_3 / conv5_3, the stride-2 upscore, the add and the dropout of
both branches):

    EmbeddingNeck(in_channels=512, num_units=64, vertex_units=128, keep_prob=0.5, seed=0)(conv4_3, conv5_3)
        -> (add_score (B,h,w,num_units), add_score_vertex (B,h,w,vertex_units))

and the backbone in front of that (posecnn_amd.backbone: the thirteen 3x3
convs and four max-pools of vgg16_convs.py:80-97; forward only):

    VGG16Convs(seed=0)(blob (B,H,W,3)) -> (conv4_3, conv5_3)
"""
import torch
from torch import nn

from .hough_voting_gpu_layer import hough_voting_gpu_op as hv
from .roi_pooling_layer import roi_pooling_op as rp
from .average_distance_loss import average_distance_loss_op as adl
from . import losses
from . import vertex_pred as vp
from . import upscore as up
from . import neck as nk
from . import backbone as bb
from . import pose_head as ph


class HoughVoting(nn.Module):
    def __init__(self, num_classes, threshold_vote, threshold_percentage, label_threshold=500, inlier_threshold=0.9,
                 skip_pixels=1, is_train=False):
        super().__init__()
        self.num_classes = int(num_classes)
        self.threshold_vote = float(threshold_vote)
        self.threshold_percentage = float(threshold_percentage)
        self.label_threshold = int(label_threshold)
        self.inlier_threshold = float(inlier_threshold)
        self.skip_pixels = int(skip_pixels)
        self.is_train = int(bool(is_train))

    def forward(self, label_2d, vertex_pred, extents, poses, meta_data):
        if vertex_pred.shape[-1] != 3 * self.num_classes:
            raise ValueError(f"vertex_pred must be NHWC with {3 * self.num_classes} channels")
        with torch.no_grad():  # the op's gradient is identically zero (hough_voting_gpu_op.cc:440-484)
            return hv.hough_voting_gpu(label_2d.to(torch.int32), vertex_pred, extents, meta_data, poses,
                                       self.is_train, self.threshold_vote, self.threshold_percentage,
                                       self.skip_pixels, inlier_threshold=self.inlier_threshold,
                                       label_threshold=self.label_threshold)


class _RoIPoolingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, rois, ph, pw, scale):
        top, arg = rp.roi_pool(features, rois, ph, pw, scale, 0, layout=1)  # NCHW, 5-column RoIs
        ctx.save_for_backward(features, rois, arg)
        ctx.params = (ph, pw, scale)
        return top

    @staticmethod
    def backward(ctx, grad):
        features, rois, arg = ctx.saved_tensors
        ph, pw, scale = ctx.params
        g = rp.roi_pool_grad(features, rois, arg, grad.contiguous(), ph, pw, scale, 0, layout=1)
        return g, None, None, None, None


class _RoIPooling(nn.Module):
    def __init__(self, pooled_height, pooled_width, spatial_scale):
        super().__init__()
        self.pooled_height = int(pooled_height)
        self.pooled_width = int(pooled_width)
        self.spatial_scale = float(spatial_scale)

    def forward(self, features, rois):
        if rois.dim() != 2 or rois.shape[1] != 5:
            raise ValueError("rois must be (N, 5): [batch, x1, y1, x2, y2]")
        return _RoIPoolingFn.apply(features.contiguous().float(), rois.contiguous().float(), self.pooled_height,
                                   self.pooled_width, self.spatial_scale)


class _SegmentationLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, gt_label_2d, threshold):
        loss, out = losses.seg_loss(score, gt_label_2d, threshold, want=("label_2d",))
        ctx.save_for_backward(score, gt_label_2d)
        ctx.threshold = threshold
        ctx.mark_non_differentiable(out["label_2d"])
        return loss, out["label_2d"]

    @staticmethod
    def backward(ctx, grad_loss, _grad_label):
        score, gt_label_2d = ctx.saved_tensors
        # the incoming gradient goes in as the op's grad_scale (a host scalar: one read-back here)
        _, out = losses.seg_loss(score, gt_label_2d, ctx.threshold, want=("d_score",), grad_scale=float(grad_loss))
        return out["d_score"].to(score.dtype), None, None


class SegmentationLoss(nn.Module):
    """loss_cls of the segmentation head: (score (B,H,W,C), gt_label_2d (B,H,W))
    -> (loss, label_2d)."""

    def __init__(self, threshold=1.0):
        super().__init__()
        if float(threshold) <= 0:
            raise ValueError(f"Need threshold > 0, got {threshold}")
        self.threshold = float(threshold)

    def forward(self, score, gt_label_2d):
        return _SegmentationLossFn.apply(score, gt_label_2d, self.threshold)


class _VertexLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertex_pred, a, b, compact, num_classes, sigma, w_inside):
        ctx.save_for_backward(vertex_pred, a, b)
        ctx.params = (compact, num_classes, sigma, w_inside)
        if compact:
            return losses.vertex_loss_compact(vertex_pred, a, b, num_classes, w_inside, sigma)
        return losses.smooth_l1_loss_vertex(vertex_pred, a, b, sigma)

    @staticmethod
    def backward(ctx, grad_loss):
        vertex_pred, a, b = ctx.saved_tensors
        compact, num_classes, sigma, w_inside = ctx.params
        g = float(grad_loss)  # as _SegmentationLossFn.backward
        if compact:
            _, d = losses.vertex_loss_compact(vertex_pred, a, b, num_classes, w_inside, sigma, want_grad=True,
                                              dense_grad=vertex_pred.shape[3] != 3, grad_scale=g)
        else:
            _, d = losses.smooth_l1_loss_vertex(vertex_pred, a, b, sigma, want_grad=True, grad_scale=g)
        return d.to(vertex_pred.dtype), None, None, None, None, None, None


class VertexLoss(nn.Module):
    """loss_vertex before the VERTEX_W factor.  forward(vertex_pred,
    vertex_targets, vertex_weights) takes the reference's blob pair;
    forward(vertex_pred, label, vertex3) takes the scene renderer's compact
    ground truth (label (B,H,W) integer, vertex3 (B,H,W,3)) with weight
    w_inside on the labelled channels.  A 3-channel vertex_pred (the compact
    producer's output) needs num_classes."""

    def __init__(self, sigma=1.0, w_inside=10.0, num_classes=None):
        super().__init__()
        if float(sigma) <= 0:
            raise ValueError(f"Need sigma > 0, got {sigma}")
        self.sigma = float(sigma)
        self.w_inside = float(w_inside)
        self.num_classes = None if num_classes is None else int(num_classes)

    def forward(self, vertex_pred, a, b):
        compact = a.dim() == 3 and not a.dtype.is_floating_point
        C = self.num_classes
        if compact and C is None:
            if vertex_pred.dim() != 4 or vertex_pred.shape[3] == 3:
                raise ValueError("a 3-channel vertex_pred needs VertexLoss(num_classes=...)")
            C = vertex_pred.shape[3] // 3
        return _VertexLossFn.apply(vertex_pred, a, b, compact, C, self.sigma, self.w_inside)


class _VertexPredCompactFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, weight, bias, label):
        ctx.save_for_backward(feat, weight, label)
        return vp.vertex_pred_compact(feat, weight, bias, label)

    @staticmethod
    def backward(ctx, grad):
        feat, weight, label = ctx.saved_tensors
        want = tuple(n for n, need in zip(vp.BWD_OUTPUTS, ctx.needs_input_grad[:3]) if need)
        if not want:
            return None, None, None, None
        d = vp.vertex_pred_compact_bwd(feat, weight, label, grad, want=want)
        like = {"feat": feat, "weights": weight, "bias": weight}
        return (*[d[n].to(like[n].dtype) if n in d else None for n in vp.BWD_OUTPUTS], None)


class VertexPredCompact(nn.Module):
    """The vertex_pred layer (vgg16_convs.py:152-163: 1x1 conv num_units -> 3C
    plus bias) evaluated at each pixel's own class: (feat (B,H,W,num_units)
    NHWC, label (B,H,W) integer) -> (B,H,W,3), differentiable in feat, weight
    and bias.  `weight` is (num_units, 3C), the reference's (1,1,K,3C) kernel
    without its two unit axes; with the ground-truth label map the gradients
    are the reference's under VertexLoss's mask."""

    def __init__(self, num_units, num_classes):
        super().__init__()
        self.num_units = int(num_units)
        self.num_classes = int(num_classes)
        self.weight = nn.Parameter(torch.empty(self.num_units, 3 * self.num_classes))
        self.bias = nn.Parameter(torch.zeros(3 * self.num_classes))
        nn.init.trunc_normal_(self.weight, std=0.001, a=-0.002, b=0.002)  # network.py:170, biases 0 (:183)

    def forward(self, feat, label):
        if feat.dim() != 4 or feat.shape[3] != self.num_units:
            raise ValueError(f"feat must be (B,H,W,{self.num_units}), got {tuple(feat.shape)}")
        return _VertexPredCompactFn.apply(feat, self.weight, self.bias, label)


class _UpscoreFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, stride, relu):
        y = up.upscore(x, stride, bias=bias, relu=relu)
        ctx.save_for_backward(*([y] if relu else []))
        ctx.params = (stride, relu, x.dtype, None if bias is None else bias.dtype)
        return y

    @staticmethod
    def backward(ctx, grad):
        stride, relu, x_dtype, b_dtype = ctx.params
        y = ctx.saved_tensors[0] if relu else None
        want_bias = b_dtype is not None and ctx.needs_input_grad[1]
        if not ctx.needs_input_grad[0] and not want_bias:
            return None, None, None, None
        d = up.upscore_bwd(grad, stride, y=y, want_bias=want_bias)
        d_x, d_b = d if want_bias else (d, None)
        return (d_x.to(x_dtype) if ctx.needs_input_grad[0] else None, d_b.to(b_dtype) if want_bias else None, None,
                None)


class Upscore(nn.Module):
    """The reference's fixed bilinear deconv (network.py:207-222 with
    trainable=False: a 2*stride square kernel at `stride`, SAME padding):
    x (B,h,w,Ch) NHWC -> (B, stride*h, stride*w, Ch).  stride 8 is `upscore` /
    `upscore_vertex`, stride 2 `upscore_conv5(_vertex)`."""

    def __init__(self, stride, relu=False):
        super().__init__()
        if stride not in up.STRIDES:
            raise ValueError(f"stride must be one of {up.STRIDES}, got {stride}")
        self.stride = int(stride)
        self.relu = bool(relu)

    def forward(self, x):
        return _UpscoreFn.apply(x, None, self.stride, self.relu)


class _UpscoreCompactFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, bias, label, stride):
        ctx.save_for_backward(label)
        ctx.params = (stride, z.shape[3] // 3, z.dtype, bias.dtype)
        return up.upscore_compact(z, bias, label, stride)

    @staticmethod
    def backward(ctx, grad):
        (label,) = ctx.saved_tensors
        stride, C, z_dtype, b_dtype = ctx.params
        want = tuple(n for n, need in zip(up.COMPACT_BWD_OUTPUTS, ctx.needs_input_grad[:2]) if need)
        if not want:
            return None, None, None, None
        d = up.upscore_compact_bwd(label, grad, C, stride, want=want)
        return (d["z"].to(z_dtype) if "z" in d else None, d["bias"].to(b_dtype) if "bias" in d else None, None, None)


class VertexHeadCompact(nn.Module):
    """`upscore_vertex` and `vertex_pred` (vgg16_convs.py:152-163) as one head
    evaluated at each pixel's own class: (x_low (B,h,w,num_units) NHWC, label
    (B, stride*h, stride*w) integer) -> (B,H,W,3).  Both layers are linear and
    the upscore is depthwise, so the 1x1 conv runs first, at low resolution
    (z = x_low @ weight, a torch matmul), and the upscore of z plus bias is
    taken at the three channels of the pixel's class.  Parameters as
    VertexPredCompact's (state dicts interchange); differentiable in x_low,
    weight and bias."""

    def __init__(self, num_units, num_classes, stride=8):
        super().__init__()
        if stride not in up.STRIDES:
            raise ValueError(f"stride must be one of {up.STRIDES}, got {stride}")
        self.num_units = int(num_units)
        self.num_classes = int(num_classes)
        self.stride = int(stride)
        self.weight = nn.Parameter(torch.empty(self.num_units, 3 * self.num_classes))
        self.bias = nn.Parameter(torch.zeros(3 * self.num_classes))
        nn.init.trunc_normal_(self.weight, std=0.001, a=-0.002, b=0.002)  # network.py:170, biases 0 (:183)

    def forward(self, x_low, label):
        if x_low.dim() != 4 or x_low.shape[3] != self.num_units:
            raise ValueError(f"x_low must be (B,h,w,{self.num_units}), got {tuple(x_low.shape)}")
        z = torch.matmul(x_low, self.weight)
        return _UpscoreCompactFn.apply(z, self.bias, label, self.stride)


class ScoreHead(nn.Module):
    """`upscore` and `score` (vgg16_convs.py:138-140: the deconv, then a 1x1
    conv num_units -> C with ReLU) with the conv first, at low resolution:
    x_low (B,h,w,num_units) -> relu(upscore(x_low @ weight) + bias), (B,H,W,C),
    the input of SegmentationLoss.  `weight` is (num_units, C)."""

    def __init__(self, num_units, num_classes, stride=8):
        super().__init__()
        if stride not in up.STRIDES:
            raise ValueError(f"stride must be one of {up.STRIDES}, got {stride}")
        self.num_units = int(num_units)
        self.num_classes = int(num_classes)
        self.stride = int(stride)
        self.weight = nn.Parameter(torch.empty(self.num_units, self.num_classes))
        self.bias = nn.Parameter(torch.zeros(self.num_classes))
        nn.init.trunc_normal_(self.weight, std=0.001, a=-0.002, b=0.002)

    def forward(self, x_low):
        if x_low.dim() != 4 or x_low.shape[3] != self.num_units:
            raise ValueError(f"x_low must be (B,h,w,{self.num_units}), got {tuple(x_low.shape)}")
        return _UpscoreFn.apply(torch.matmul(x_low, self.weight), self.bias, self.stride, True)


class _EmbeddingNeckFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x4, x5, W4, b4, W5, b5, num_units, keep_prob, drop_gen):
        s, v, c = nk.embedding(x4, x5, W4, b4, W5, b5, num_units, keep_prob=keep_prob, drop_gen=drop_gen)
        ctx.save_for_backward(x4, x5, W4, b4, W5, b5, c["z4"], c["z5"], c["keep_score"], c["keep_vertex"])
        ctx.params = (c["num_units"], c["keep_prob"], c["precision"])
        return s, v

    @staticmethod
    def backward(ctx, grad_s, grad_v):
        x4, x5, W4, b4, W5, b5, z4, z5, keep_s, keep_v = ctx.saved_tensors
        U, kp, prec = ctx.params
        want = tuple(n for n, need in zip(nk.BWD_OUTPUTS, ctx.needs_input_grad[:6]) if need)
        if not want:
            return (None,) * 9
        c = dict(x4=x4, x5=x5, W4=W4, W5=W5, b4=b4, b5=b5, z4=z4, z5=z5, keep_score=keep_s, keep_vertex=keep_v,
                 num_units=U, keep_prob=kp, precision=prec)
        d = nk.embedding_bwd(c, grad_s.contiguous(), grad_v.contiguous(), want=want)
        return (*[d.get(n) for n in nk.BWD_OUTPUTS], None, None, None)


class EmbeddingNeck(nn.Module):
    """The layers between conv4_3 / conv5_3 and the two heads
    (vgg16_convs.py:128-137 and :152-161: score_conv5, upscore_conv5,
    score_conv4, add_score, dropout and their _vertex twins) as one layer
    group over posecnn_amd.neck: (conv4_3 (B,h,w,in_channels), conv5_3
    (B,h/2,w/2,in_channels)) NHWC float32, h and w even -> (add_score
    (B,h,w,num_units), add_score_vertex (B,h,w,vertex_units)), the inputs of
    ScoreHead and VertexHeadCompact.  weight4, weight5 are (in_channels,
    num_units + vertex_units), the score branch's columns (ReLU) first, the
    reference's four (1,1,K,units) kernels side by side; bias4, bias5 likewise.
    Dropout draws from (seed, the module's device-side step counter, one Philox
    stream per branch): call advance() once per training step; eval() means
    keep_prob = 1 and draws nothing."""

    def __init__(self, in_channels=512, num_units=64, vertex_units=128, keep_prob=0.5, seed=0):
        super().__init__()
        self.in_channels, self.num_units, self.vertex_units = int(in_channels), int(num_units), int(vertex_units)
        if self.num_units < 0 or self.vertex_units < 0 or self.num_units % 4 or self.vertex_units % 4 or \
                self.num_units + self.vertex_units == 0:
            raise ValueError(f"num_units and vertex_units must be multiples of 4, not both 0, got {num_units}, "
                             f"{vertex_units}")
        if not 0.0 < float(keep_prob) <= 1.0:
            raise ValueError(f"Need keep_prob in (0, 1], got {keep_prob}")
        self.keep_prob, self.seed = float(keep_prob), int(seed)
        N = self.num_units + self.vertex_units
        g = torch.Generator(device="cpu")
        g.manual_seed(self.seed)
        init = lambda: nn.Parameter(ph.truncated_normal((self.in_channels, N), 0.001, g, "cpu"))  # noqa: E731
        self.weight4, self.weight5 = init(), init()  # network.py:170, biases 0 (:183)
        self.bias4, self.bias5 = nn.Parameter(torch.zeros(N)), nn.Parameter(torch.zeros(N))
        self.register_buffer("step", torch.zeros(1, dtype=torch.int64))

    def advance(self):
        """Bump the device-side step counter: the next forward draws fresh masks (no sync)."""
        self.step += 1

    def forward(self, conv4_3, conv5_3):
        kp = self.keep_prob if self.training else 1.0
        drop_gen = (self.seed, self.step, nk.STREAM_IDS) if kp < 1.0 else None
        return _EmbeddingNeckFn.apply(conv4_3, conv5_3, self.weight4, self.bias4, self.weight5, self.bias5,
                                      self.num_units, kp, drop_gen)

    @torch.no_grad()
    def load_reference(self, score_conv4, score_conv5, score_conv4_vertex, score_conv5_vertex):
        """Each argument is the reference variable pair (weights (1,1,K,units) or
        (K,units), biases (units)) of the layer of that name; a branch with no
        columns takes None."""
        def cat(score, vertex, what):
            parts = []
            for pair, units in ((score, self.num_units), (vertex, self.vertex_units)):
                if units:
                    t = torch.as_tensor(pair[what], dtype=torch.float32)
                    parts.append(t.reshape(-1, units) if what == 0 else t.reshape(units))
            return torch.cat(parts, dim=-1)
        for name, score, vertex, what in (("weight4", score_conv4, score_conv4_vertex, 0),
                                          ("bias4", score_conv4, score_conv4_vertex, 1),
                                          ("weight5", score_conv5, score_conv5_vertex, 0),
                                          ("bias5", score_conv5, score_conv5_vertex, 1)):
            p = getattr(self, name)
            v = cat(score, vertex, what)
            if v.shape != p.shape:
                raise ValueError(f"{name}: expected shape {tuple(p.shape)}, got {tuple(v.shape)}")
            p.copy_(v)


class _ConvVars(nn.Module):
    """The variable pair of one conv layer under the reference's names (network.py:170, :183)."""

    def __init__(self, cin, cout, generator):
        super().__init__()
        self.weights = nn.Parameter(ph.truncated_normal((3, 3, cin, cout), 0.001, generator, "cpu"),
                                    requires_grad=False)
        self.biases = nn.Parameter(torch.zeros(cout), requires_grad=False)


class VGG16Convs(nn.Module):
    """The backbone of vgg16_convs.py:80-97 over posecnn_amd.backbone: blob
    (B,H,W,3) NHWC float32 -> (conv4_3 (B,ceil(H/8),ceil(W/8),512), conv5_3
    (B,ceil(H/16),ceil(W/16),512)), the inputs of EmbeddingNeck (which wants
    H and W multiples of 16).  Parameters are the reference's variables under
    its names, conv1_1.weights (3,3,3,64) HWIO, conv1_1.biases (64), ...,
    initialised as the reference does (truncated normal, stddev 0.001; zero
    biases).  Forward only: the parameters are created with
    requires_grad=False, and forward raises NotImplementedError rather than
    hand back zero gradients if the input or a parameter requires grad."""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator(device="cpu")
        g.manual_seed(int(seed))
        for name, cin, cout in bb.CONVS:
            setattr(self, name, _ConvVars(cin, cout, g))

    def params(self):
        return {name: (getattr(self, name).weights, getattr(self, name).biases) for name, _, _ in bb.CONVS}

    def forward(self, blob, keep=()):
        needs = [n for n, p in self.named_parameters() if p.requires_grad]
        if blob.requires_grad or needs:
            what = "the input" if blob.requires_grad else needs[0]
            raise NotImplementedError(f"VGG16Convs: {what} requires grad, but the backward of the 3x3 conv and the "
                                      "max-pool is not built; detach the input and keep requires_grad=False")
        with torch.no_grad():
            return bb.vgg16_convs(blob, self.params(), keep=keep)

    @torch.no_grad()
    def load_reference(self, **layers):
        """load_reference(conv1_1=(weights (3,3,3,64), biases (64)), ...): the
        reference's variable pairs by layer name, any subset of the thirteen."""
        known = {name: (cin, cout) for name, cin, cout in bb.CONVS}
        for name, pair in layers.items():
            if name not in known:
                raise ValueError(f"load_reference: unknown layer {name}; expected one of {tuple(known)}")
            mod = getattr(self, name)
            for p, v, what in ((mod.weights, pair[0], "weights"), (mod.biases, pair[1], "biases")):
                v = torch.as_tensor(v, dtype=torch.float32)
                if v.shape != p.shape:
                    raise ValueError(f"{name}.{what}: expected shape {tuple(p.shape)}, got {tuple(v.shape)}")
                p.copy_(v)


class AverageDistanceLoss(nn.Module):
    def __init__(self, num_classes, margin=0.01):
        super().__init__()
        self.num_classes = int(num_classes)
        self.margin = float(margin)

    def forward(self, poses_pred, poses_target, poses_weight, points, symmetry):
        if poses_pred.shape[1] != 4 * self.num_classes:
            raise ValueError(f"poses_pred must have {4 * self.num_classes} columns")
        return adl.AverageDistanceFunction.apply(poses_pred, poses_target, poses_weight, points, symmetry,
                                                 self.margin)
