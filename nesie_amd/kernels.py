"""Kernel back end used by ``nesie_amd.mmdet3d_ops``.

The product back end is :class:`HipKernels` (libnesie_hip.so on the current HIP
stream).  ``use_backend`` lets TEST CODE and bench.py's cpu_baseline leg inject
another object with the same methods (the CPU oracle lives outside this
package, under ``oracle/``); nothing in nesie_amd ever installs one, and
without an injected back end a non-HIP tensor is an error, not a fallback.

Method names and argument order are those of the reference's extension
modules; every tensor must be contiguous; outputs are
pre-allocated by the caller and written in place.
"""
import contextlib
import os

import ctypes

import torch

from . import _lib

_injected = None


def _no_cpu_path(device):
    return RuntimeError(
        "nesie_amd kernels need HIP device tensors (got device "
        f"{device}); there is no CPU path in the product")


def _check(*tensors):
    for t in tensors:
        if not t.is_cuda:
            raise _no_cpu_path(t.device)
        if not t.is_contiguous():
            raise RuntimeError("nesie_amd kernels need contiguous tensors")


def _f32(*ts):
    for t in ts:
        if t.dtype != torch.float32:
            raise TypeError(f"expected float32, got {t.dtype}")


def _i32(*ts):
    for t in ts:
        if t.dtype != torch.int32:
            raise TypeError(f"expected int32, got {t.dtype}")


def _launch(name, on, *args):
    """Call the entry point ``name`` on the device and current stream of ``on`` (a tensor, or the
    torch.device itself for a call without tensors); the stream is appended as the last argument.
    A tensor is passed as its address, None as a null pointer, a bool as 0 / 1.  The call is
    checked against the header's prototype first: the argument count, and no tensor or None
    outside a pointer slot, no float inside one."""
    argtypes = _lib.SIGNATURES[name][1]
    if len(args) + 1 != len(argtypes):
        raise TypeError(f"{name}: {len(args)} arguments and the stream given, "
                        f"the header declares {len(argtypes)}")
    out = []
    for slot, (a, ctype) in enumerate(zip(args, argtypes)):
        if a is None or isinstance(a, torch.Tensor):
            if ctype is not ctypes.c_void_p:
                raise TypeError(f"{name}: argument {slot} is a {ctype.__name__} in the header, got "
                                + ("None" if a is None else "a tensor"))
            a = 0 if a is None else a.data_ptr()
        elif ctype is ctypes.c_void_p and isinstance(a, float):
            raise TypeError(f"{name}: argument {slot} is a pointer in the header, got a float")
        elif isinstance(a, bool):
            a = int(a)
        out.append(a)
    device = on.device if isinstance(on, torch.Tensor) else on
    if device.type != "cuda":
        raise _no_cpu_path(device)
    with torch.cuda.device(device):
        _lib.call(name, *out, torch.cuda.current_stream(device).cuda_stream)


def _workspace(need, device):
    """``need`` bytes of kernel scratch from torch's caching allocator (never an empty tensor)."""
    return torch.empty(max(need, 16), dtype=torch.uint8, device=device)


def blend_backward_form(c, per_seg, m, deterministic):
    """Which blend backward serves c channels, per_seg queries per face and m seeds:
    'staged' (nesie_blend_conv_backward_staged: the 64 x 64-tile shapes, c in 64..256 step 64, whole
    64-query tiles per face, at most 2047 seeds; fixed order), 'atomic' (the same tile shapes with
    float atomics, when the deterministic backward is off) or 'any' (nesie_blend_conv_backward_any:
    everything else, in both modes; fixed order)."""
    tile = c % 64 == 0 and 64 <= c <= 256 and per_seg > 0 and per_seg % 64 == 0
    if not tile:
        return 'any'
    if not deterministic:
        return 'atomic'
    return 'staged' if m + 1 <= 2048 else 'any'


class HipKernels:
    """libnesie_hip.so, asynchronous on torch's current HIP stream."""

    name = "hip"

    # The bucket-pruned FPS kernel leaves the scene spatially sorted in its scratch; the ball
    # query that follows on the SAME coordinates (every set-abstraction module samples and then
    # groups one cloud) can use it as an index.  The hand-over is scoped: an entry is recorded
    # only inside ``spatial_index_scope()`` -- one set-abstraction forward -- and dropped when the
    # scope ends, so a ball query somewhere else can never meet the index of an earlier scene
    # (a buffer refilled by a kernel, a memcpy or a graph replay keeps its address AND its
    # version counter).  Inside the scope the entry keeps the coordinate tensor alive and still
    # records address, version, shape, stream and capture state.  One entry per device.
    _spatial_index = {}
    _index_scope_depth = 0

    @staticmethod
    def set_distance_form(form):
        """Process-wide form of the squared distance in FPS / ball query / 3-NN / grid taps
        (include/nesie_ops.h ``nesie_set_distance_form``): 0 = contraction-free (default, the
        tuned kernels), 1 / 2 = the fused forms an nvcc build of the reference may compute."""
        _lib.call("nesie_set_distance_form", int(form))

    @staticmethod
    def get_distance_form():
        return _lib.load().nesie_get_distance_form()

    @staticmethod
    @contextlib.contextmanager
    def cu_budget(n):
        """Inside: the persistent grids of the layer / weight-gradient kernels are sized for ``n``
        CUs instead of the chip's 256 (``nesie_set_cu_count``) -- for launches that run beside
        long-lived workgroups of another stream (the next batch's furthest point sampling holds
        one CU per scene and XCD).  Host-side sizing only: a captured graph keeps what it was
        captured with."""
        lib = _lib.load()
        before = lib.nesie_get_cu_count()
        _lib.call("nesie_set_cu_count", int(n))
        try:
            yield
        finally:
            _lib.call("nesie_set_cu_count", before)

    @staticmethod
    def _stream_state(device):
        """(current stream of ``device``, whether a graph capture is recording it)."""
        with torch.cuda.device(device):   # is_current_stream_capturing() reads the current device
            return (torch.cuda.current_stream(device).cuda_stream,
                    torch.cuda.is_current_stream_capturing())

    @classmethod
    def _index_for(cls, xyz, b, n):
        hit = cls._spatial_index.get(xyz.device)
        if hit is None:
            return None
        ref, version, shape, ws, stream, capturing = hit
        # an entry made while a graph was being captured describes that graph's static buffers:
        # replays rewrite them without touching the version counter, so eager code must not
        # trust it (and vice versa)
        same = (ref.data_ptr() == xyz.data_ptr() and ref._version == version
                and xyz._version == version and shape == (b, n) and ref.dtype == xyz.dtype
                and (stream, capturing) == cls._stream_state(xyz.device))
        return ws if same else None

    def furthest_point_sampling_wrapper(self, b, n, m, xyz, temp, idx):
        _check(xyz, temp, idx); _f32(xyz, temp); _i32(idx)
        assert xyz.numel() == b * n * 3 and temp.numel() == b * n and idx.numel() == b * m
        lib = _lib.load()
        need = lib.nesie_fps_workspace_bytes(b, n)
        if need:
            # scratch for the bucket-pruned kernel, from torch's caching allocator
            ws = torch.empty(need, dtype=torch.uint8, device=xyz.device)
            _launch("nesie_furthest_point_sampling_ws", xyz, b, n, m, xyz, temp, idx, ws, need)
            if HipKernels._index_scope_depth > 0 and lib.nesie_fps_leaves_index(b, n):
                HipKernels._spatial_index[xyz.device] = (
                    xyz, xyz._version, (b, n), ws, *self._stream_state(xyz.device))
        else:
            _launch("nesie_furthest_point_sampling_wrapper", xyz, b, n, m, xyz, temp, idx)

    def furthest_point_sampling_with_dist_wrapper(self, b, n, m, dist, temp, idx):
        _check(dist, temp, idx); _f32(dist, temp); _i32(idx)
        assert dist.numel() == b * n * n and temp.numel() == b * n and idx.numel() == b * m
        _launch("nesie_furthest_point_sampling_with_dist_wrapper", dist, b, n, m, dist, temp, idx)

    def ball_query_wrapper(self, b, n, m, min_radius, max_radius, nsample, new_xyz, xyz,
                           idx):
        _check(new_xyz, xyz, idx); _f32(new_xyz, xyz); _i32(idx)
        assert new_xyz.numel() == b * m * 3 and xyz.numel() == b * n * 3
        assert idx.numel() == b * m * nsample
        ws = self._index_for(xyz, b, n) if nsample <= 64 else None
        if ws is not None:  # same results, only the buckets within max_radius are visited
            _launch("nesie_ball_query_indexed", xyz, b, n, m, float(min_radius), float(max_radius),
                    nsample, new_xyz, ws, ws.numel(), idx)
            return
        _launch("nesie_ball_query_wrapper", xyz, b, n, m, float(min_radius), float(max_radius),
                nsample, new_xyz, xyz, idx)

    def knn_wrapper(self, b, n, m, nsample, xyz, new_xyz, idx, dist2):
        """idx, dist2 (B, M, nsample) <- the nsample nearest points of every centre, ascending in
        (squared distance, point index) (nesie_knn_wrapper)."""
        _check(xyz, new_xyz, idx, dist2); _f32(xyz, new_xyz, dist2); _i32(idx)
        assert xyz.numel() == b * n * 3 and new_xyz.numel() == b * m * 3
        assert idx.numel() == b * m * nsample and dist2.numel() == b * m * nsample
        _launch("nesie_knn_wrapper", xyz, b, n, m, nsample, xyz, new_xyz, idx, dist2)

    def group_points_forward(self, b, c, n, npoints, nsample, points, idx, out):
        _check(points, idx, out); _f32(points, out); _i32(idx)
        assert points.numel() == b * c * n and idx.numel() == b * npoints * nsample
        assert out.numel() == b * c * npoints * nsample
        _launch("nesie_group_points_forward", points, b, c, n, npoints, nsample, points, idx, out)

    def group_points_backward(self, b, c, n, npoints, nsample, grad_out, idx, grad_points):
        _check(grad_out, idx, grad_points); _f32(grad_out, grad_points); _i32(idx)
        assert grad_out.numel() == b * c * npoints * nsample
        assert idx.numel() == b * npoints * nsample and grad_points.numel() == b * c * n
        _launch("nesie_group_points_backward", grad_out, b, c, n, npoints, nsample, grad_out, idx,
                grad_points)

    def gather_points_wrapper(self, b, c, n, npoints, points, idx, out):
        _check(points, idx, out); _f32(points, out); _i32(idx)
        assert points.numel() == b * c * n and idx.numel() == b * npoints
        assert out.numel() == b * c * npoints
        _launch("nesie_gather_points_wrapper", points, b, c, n, npoints, points, idx, out)

    def gather_points_grad_wrapper(self, b, c, n, npoints, grad_out, idx, grad_points):
        _check(grad_out, idx, grad_points); _f32(grad_out, grad_points); _i32(idx)
        assert grad_out.numel() == b * c * npoints and idx.numel() == b * npoints
        assert grad_points.numel() == b * c * n
        _launch("nesie_gather_points_grad_wrapper", grad_out, b, c, n, npoints, grad_out, idx,
                grad_points)

    def query_and_group_forward(self, xyz, centres, features, idx, radius, out):
        """out (B, 3+C, M, ns) = cat[(xyz[idx] - centre) / radius, features[idx]]."""
        _check(xyz, centres, idx, out); _f32(xyz, centres, out); _i32(idx)
        b, n = xyz.shape[:2]
        m, ns = idx.shape[1], idx.shape[2]
        c = 0 if features is None else features.shape[1]
        if features is not None:
            _check(features); _f32(features)
            assert tuple(features.shape) == (b, c, n)
        assert tuple(out.shape) == (b, 3 + c, m, ns) and tuple(centres.shape) == (b, m, 3)
        _launch("nesie_query_and_group_forward", xyz, b, c, n, m, ns, xyz, centres, features, idx,
                float(radius), out)

    def query_and_group_backward(self, grad_out, idx, grad_features):
        """grad_features (B,C,N) zeroed += channels 3.. of grad_out (B, 3+C, M, ns)."""
        _check(grad_out, idx, grad_features); _f32(grad_out, grad_features); _i32(idx)
        b, c, n = grad_features.shape
        m, ns = idx.shape[1], idx.shape[2]
        assert tuple(grad_out.shape) == (b, 3 + c, m, ns)
        _launch("nesie_query_and_group_backward", grad_out, b, c, n, m, ns, grad_out, idx,
                grad_features)

    def three_interpolate_grad_csr(self, grad_out, weight, order, sources, grad_points):
        """grad_points (B,C,m) = scatter of weight * grad_out (B,C,n) through (order, sources) =
        inverted_index(idx (B,n,3), m); WRITTEN in full (no zero fill needed).  grad_out may be a
        channel slice of a wider tensor (batch stride free, rows contiguous)."""
        _check(weight, order, sources, grad_points); _f32(grad_out, weight, grad_points)
        _i32(order, sources)
        b, c, n = grad_out.shape
        m = grad_points.shape[2]
        assert grad_out.is_cuda and grad_out.stride(2) == 1 and grad_out.stride(1) == n
        assert weight.numel() == b * n * 3 and tuple(order.shape) == (b, n * 3)
        _launch("nesie_three_interpolate_grad_csr", grad_out, b, c, n, m, grad_out,
                grad_out.stride(0) if b > 1 else c * n, weight, order, sources, grad_points)

    def inverted_index(self, idx, n):
        """idx (B, M, ns) int32 in [0, n) -> order, sources (B, M*ns) int32: the grouped columns
        sorted by source point (ascending column inside a point's run) and that point for each."""
        _check(idx); _i32(idx)
        b = idx.shape[0]
        e = idx.numel() // b
        order = torch.empty(b, e, dtype=torch.int32, device=idx.device)
        sources = torch.empty(b, e, dtype=torch.int32, device=idx.device)
        scratch = torch.empty(b, e, dtype=torch.int32, device=idx.device)
        _launch("nesie_inverted_index", idx, b, n, e, idx, order, sources, scratch)
        return order, sources

    def vote_finish_forward(self, raw, seed_points, seed_feats, normalise):
        """-> (vote_points (B, N, 3), vote_feats (B, C, N), inv_norm (B, N)) (nesie_vote_finish_forward)."""
        _check(raw, seed_points, seed_feats); _f32(raw, seed_points, seed_feats)
        b, c, n = seed_feats.shape
        assert tuple(raw.shape) == (b, 3 + c, n) and tuple(seed_points.shape) == (b, n, 3)
        vp, vf = torch.empty_like(seed_points), torch.empty_like(seed_feats)
        inv = torch.empty(b, n, dtype=torch.float32, device=raw.device)
        _launch("nesie_vote_finish_forward", raw, b, c, n, bool(normalise), raw, seed_points,
                seed_feats, vp, vf, inv)
        return vp, vf, inv

    def vote_finish_backward(self, g_feats, g_points, vote_feats, inv_norm, normalise):
        """-> d_raw (B, 3 + C, N) (nesie_vote_finish_backward); either gradient may be None."""
        _check(vote_feats, inv_norm); _f32(vote_feats, inv_norm)
        b, c, n = vote_feats.shape
        for t, shape in ((g_feats, (b, c, n)), (g_points, (b, n, 3))):
            if t is not None:
                _check(t); _f32(t)
                assert tuple(t.shape) == shape
        d_raw = torch.empty(b, 3 + c, n, dtype=torch.float32, device=vote_feats.device)
        _launch("nesie_vote_finish_backward", vote_feats, b, c, n, bool(normalise), g_feats,
                g_points, vote_feats, inv_norm, d_raw)
        return d_raw

    def gather_rows3(self, xyz, sample):
        """xyz (B, N, 3), sample (B, M) int32 -> xyz[b, sample[b, m]] (B, M, 3)."""
        _check(xyz, sample); _f32(xyz); _i32(sample)
        b, n = xyz.shape[:2]
        m = sample.shape[1]
        out = torch.empty(b, m, 3, dtype=torch.float32, device=xyz.device)
        _launch("nesie_gather_rows3", xyz, b, n, m, xyz, sample, out)
        return out

    def query_and_group_backward_xyz(self, grad_out, radius, order, sources, sample, d_centres, n):
        """Coordinate gradient (B, N, 3) of QueryAndGroup over network-computed coordinates whose
        centres are xyz[sample] (nesie_query_and_group_backward_xyz); grad_out (B, 3+C, M, ns),
        d_centres (B, M, 3) or None."""
        _check(grad_out, order, sources, sample); _f32(grad_out); _i32(order, sources, sample)
        b, c3, m, ns = grad_out.shape
        assert tuple(order.shape) == (b, m * ns) == tuple(sources.shape) and tuple(sample.shape) == (b, m)
        if d_centres is not None:
            _check(d_centres); _f32(d_centres)
            assert tuple(d_centres.shape) == (b, m, 3)
        d_xyz = torch.empty(b, n, 3, dtype=torch.float32, device=grad_out.device)
        _launch("nesie_query_and_group_backward_xyz", grad_out, b, c3 - 3, n, m, ns, float(radius),
                grad_out, order, sources, sample, d_centres, d_xyz)
        return d_xyz

    def query_and_group_backward_csr(self, grad_out, idx_shape, order, offsets, grad_features):
        """grad_features (B,C,N) = scatter of channels 3.. of grad_out through (order, sources);
        WRITTEN in full (no zero fill needed)."""
        _check(grad_out, order, offsets, grad_features); _f32(grad_out, grad_features)
        _i32(order, offsets)
        b, c, n = grad_features.shape
        m, ns = idx_shape[1], idx_shape[2]
        assert tuple(grad_out.shape) == (b, 3 + c, m, ns)
        assert tuple(order.shape) == (b, m * ns) and tuple(offsets.shape) == (b, m * ns)
        _launch("nesie_query_and_group_backward_csr", grad_out, b, c, n, m, ns, grad_out, order,
                offsets, grad_features)

    def group_points_backward_csr(self, grad_out, order, sources, grad_points):
        """grad_points (B,C,N) = scatter of grad_out (B,C,M,ns) through (order, sources) =
        inverted_index(idx (B,M,ns), N): no float atomics, WRITTEN in full
        (nesie_group_points_backward_csr)."""
        _check(grad_out, order, sources, grad_points); _f32(grad_out, grad_points); _i32(order, sources)
        b, c, n = grad_points.shape
        m, ns = grad_out.shape[2], grad_out.shape[3]
        assert grad_out.shape[:2] == (b, c) and tuple(order.shape) == (b, m * ns) == tuple(sources.shape)
        _launch("nesie_group_points_backward_csr", grad_out, b, c, n, m, ns, grad_out, order,
                sources, grad_points)

    def three_nn_wrapper(self, b, n, m, unknown, known, dist2, idx):
        _check(unknown, known, dist2, idx); _f32(unknown, known, dist2); _i32(idx)
        assert unknown.numel() == b * n * 3 and known.numel() == b * m * 3
        assert dist2.numel() == b * n * 3 and idx.numel() == b * n * 3
        _launch("nesie_three_nn_wrapper", unknown, b, n, m, unknown, known, dist2, idx)

    def three_interpolate_wrapper(self, b, c, m, n, points, idx, weight, out):
        _check(points, idx, weight, out); _f32(points, weight, out); _i32(idx)
        assert points.numel() == b * c * m and idx.numel() == b * n * 3
        assert weight.numel() == b * n * 3 and out.numel() == b * c * n
        _launch("nesie_three_interpolate_wrapper", points, b, c, m, n, points, idx, weight, out)

    def side_decode_forward(self, reg, agg, scale, sign, probs, surface, bbox):
        _check(reg, agg, scale, sign, probs, surface, bbox); _f32(reg, agg, probs, surface, bbox)
        b, cch, k = reg.shape
        bins = (cch - 2) // 6
        assert tuple(probs.shape) == (b, 6, bins, k) and tuple(bbox.shape) == (b, k, 7)
        _launch("nesie_side_decode_forward", reg, b, k, bins, reg, agg, scale, sign, probs, surface,
                bbox)

    def side_decode_backward(self, reg, probs, scale, sign, d_surface, d_bbox, d_reg, d_agg):
        _check(reg, probs, scale, sign, d_reg, d_agg)
        b, cch, k = reg.shape
        bins = (cch - 2) // 6
        for t in (d_surface, d_bbox):
            if t is not None:
                _check(t); _f32(t)
        _launch("nesie_side_decode_backward", reg, b, k, bins, reg, probs, scale, sign, d_surface,
                d_bbox, d_reg, d_agg)

    def bn_eval_coef(self, gamma, beta, running_mean, running_var, eps, coef):
        """coef (C,4) <- (gamma / sqrt(var + eps), beta - mean * scale, 0, 0); one launch."""
        _check(running_mean, running_var, coef); _f32(running_mean, running_var, coef)
        c = running_mean.numel()
        assert tuple(coef.shape) == (c, 4) and coef.is_contiguous()
        _launch("nesie_bn_eval_coef", coef, c, gamma, beta, running_mean, running_var, float(eps),
                coef)

    def affine_relu_forward(self, x, coef, relu, y, row_bias=None):
        """Evaluation-mode norm: y = relu?(coef[c,0] * (x + row_bias) + coef[c,1]); x, y (B,C,*)."""
        _check(x, coef, y); _f32(x, coef, y)
        b, c = x.shape[:2]
        p = x.numel() // (b * c) if b * c else 0
        assert tuple(coef.shape) == (c, 4) and y.shape == x.shape
        group = _row_bias_group(x, row_bias)
        _launch("nesie_affine_relu_forward", x, b, c, p, x, coef, bool(relu), row_bias, group, y)

    def affine_relu_maxpool_forward(self, x, coef, pooled, argmax):
        """x (B,C,M,ns) -> pooled (B,C,M) = max_ns relu(coef[c,0] * x + coef[c,1]), argmax u8."""
        _check(x, coef, pooled, argmax); _f32(x, coef, pooled)
        b, c, m, ns = x.shape
        assert tuple(coef.shape) == (c, 4) and tuple(pooled.shape) == (b, c, m)
        assert argmax.dtype == torch.uint8 and tuple(argmax.shape) == (b, c, m)
        _launch("nesie_affine_relu_maxpool_forward", x, b, c, m, ns, x, coef, pooled, argmax)

    def mlp_stream_forward(self, x, w, y, stat_partial=None, in_coef=None, in_relu=False):
        """y[b] = W . act(x[b]) on the matrix cores, streaming form (Cin <= 64, Cout <= 128):
        x (B,Cin,P), w (Cout,Cin), y (B,Cout,P); stat_partial (parts, Cout, 2) receives the
        per-workgroup (sum, sum of squares) of y, parts = mlp_stream_parts(B, P)."""
        _check(x, w); _f32(x, w)
        b, cin, p = x.shape
        cout = w.shape[0]
        assert tuple(w.shape) == (cout, cin)
        if y is not None:       # (None: only the statistics of y are wanted)
            _check(y); _f32(y)
            assert tuple(y.shape) == (b, cout, p)
        else:
            assert stat_partial is not None
        if stat_partial is not None:
            _check(stat_partial); _f32(stat_partial)
            assert tuple(stat_partial.shape) == (self.mlp_stream_parts(b, p), cout, 2)
        _launch("nesie_mlp_layer_forward_stream", x, b, cin, cout, p, x, cin * p, w, in_coef,
                bool(in_relu), y, stat_partial)

    @staticmethod
    def mlp_stream_parts(b, p):
        return int(_lib.load().nesie_mlp_stream_partials(b, p))

    def aligned_3d_nms(self, boxes, scores, classes, valid, thr, picks, count):
        """boxes (B,K,6), scores (B,K), classes (B,K) i32, valid (B,K) u8 or None ->
        picks (B,K) i32 (-1 padded, pick order), count (B) i32."""
        _check(boxes, scores, classes, picks, count); _f32(boxes, scores); _i32(classes, picks, count)
        b, k = scores.shape
        assert tuple(boxes.shape) == (b, k, 6) and tuple(classes.shape) == (b, k)
        assert tuple(picks.shape) == (b, k) and count.numel() == b
        if valid is not None:
            _check(valid)
            assert valid.dtype == torch.uint8 and tuple(valid.shape) == (b, k)
        _launch("nesie_aligned_3d_nms", boxes, b, k, boxes, scores, classes, valid, float(thr),
                picks, count)

    def points_in_boxes_count(self, boxes, pts, counts):
        """boxes (B,T,7) LiDAR frame, pts (B,M,3) -> counts (B,T) i32."""
        _check(boxes, pts, counts); _f32(boxes, pts); _i32(counts)
        b, t, _ = boxes.shape
        assert pts.shape[0] == b and pts.shape[2] == 3 and tuple(counts.shape) == (b, t)
        _launch("nesie_points_in_boxes_count", boxes, b, t, pts.shape[1], boxes, pts, counts)

    def boxes_overlap_bev(self, boxes_a, boxes_b, ans_overlap):
        """(N,5), (M,5) rotated BEV rectangles (x1,y1,x2,y2,angle) -> overlap areas (N,M)."""
        _check(boxes_a, boxes_b, ans_overlap); _f32(boxes_a, boxes_b, ans_overlap)
        n, m = boxes_a.shape[0], boxes_b.shape[0]
        assert boxes_a.shape[1] == 5 and boxes_b.shape[1] == 5
        assert tuple(ans_overlap.shape) == (n, m)
        _launch("nesie_boxes_overlap_bev", boxes_a, n, boxes_a, m, boxes_b, ans_overlap)

    def bev_nms(self, boxes, scores, valid, offsets, max_seg, thr, rotated, keep, count, ws):
        """(n,5) (x1,y1,x2,y2,ry), scores (n), valid (n) u8 or None, offsets (S+1) i32 ->
        keep (n) i32 (kept rows of segment t from offsets[t], best first), count (S) i32."""
        _check(boxes, scores, offsets, keep, count, ws); _f32(boxes, scores); _i32(offsets, keep, count)
        n, s = scores.numel(), count.numel()
        assert tuple(boxes.shape) == (n, 5) and offsets.numel() == s + 1 and keep.numel() == n
        if valid is not None:
            _check(valid)
            assert valid.dtype == torch.uint8 and valid.numel() == n
        _launch("nesie_bev_nms", boxes, n, s, int(max_seg), boxes, scores, valid, offsets,
                float(thr), 1 if rotated else 0, keep, count, ws, ws.numel() * ws.element_size())

    def scene_assemble(self, pool, height, choices, xform, out):
        """pool (R,3), height (R), choices (B,n) i32 rows of the pool, xform (B,20) -> out (B,n,4)."""
        _check(pool, height, choices, xform, out); _f32(pool, height, xform, out); _i32(choices)
        b, n = choices.shape
        assert pool.dim() == 2 and pool.shape[1] == 3 and height.numel() == pool.shape[0]
        assert tuple(xform.shape) == (b, 20) and tuple(out.shape) == (b, n, 4)
        _launch("nesie_scene_assemble", pool, b, n, pool.shape[0], pool, height, choices, xform,
                out)

    def grid_taps(self, centre, size, heading, mult, plane, known):
        """-> idx (B,K*gp,3) int32, weight, rel (B,K*gp,3) for the gp grid points per proposal."""
        _check(centre, size, heading, mult, plane, known)
        _f32(centre, size, heading, mult, plane, known)
        b, k = centre.shape[:2]
        gp, m = mult.shape[0], known.shape[1]
        assert tuple(size.shape) == (b, k, 3) and tuple(heading.shape) == (b, k)
        assert tuple(plane.shape) == (gp, 3) and known.shape[0] == b
        idx = torch.empty(b, k * gp, 3, dtype=torch.int32, device=centre.device)
        weight = torch.empty(b, k * gp, 3, dtype=torch.float32, device=centre.device)
        rel = torch.empty_like(weight)
        _launch("nesie_grid_taps", centre, b, k, gp, m, centre, size, heading, mult, plane, known,
                idx, weight, rel)
        return idx, weight, rel

    def blend_conv_forward(self, table, seg_off, idx, weight, rel, wx, out, segs, seg_len,
                           c, c_offset, stat_partial=None):
        """table (B, M, pitch) point-major; out (B, segs, c_total, n/segs): query (k, s, g) ->
        out[b, s, c_offset+ch, k*seg_len+g] = blend(table[..., s*seg_off+ch]) (+ wx[s,ch].rel)."""
        _check(table, idx, weight, out); _f32(table, weight, out); _i32(idx)
        b, m, pitch = table.shape
        n = idx.shape[1]
        assert idx.numel() == b * n * 3 and weight.numel() == b * n * 3
        assert n % (segs * seg_len) == 0 and out.dim() == 4
        assert out.shape[0] == b and out.shape[1] == segs and out.shape[3] * segs == n
        assert c_offset + c <= out.shape[2] and (rel is None) == (wx is None)
        if wx is not None:
            _check(rel, wx); _f32(rel, wx)
            assert rel.numel() == b * n * 3 and tuple(wx.shape) == (segs, c, 3)
        if stat_partial is not None:
            _check(stat_partial); _f32(stat_partial)
            assert stat_partial.numel() == segs * c * (b * (n // segs // 64)) * 2
        _launch("nesie_blend_conv_forward", table, b, c, m, n, table, pitch, seg_off, idx, weight,
                rel, wx, out, segs, seg_len, int(out.shape[2]), c_offset, stat_partial)

    # Deterministic backward -- THE DEFAULT since round 5 (NESIE_DETERMINISTIC=0 or
    # ``set_deterministic(False)`` restores the reference's atomicAdd scatters,
    # three_interpolate_cuda.cu:61-84, group_points_cuda.cu:10-31): every scatter-add of the backward
    # pass runs in an order fixed by the indices alone --
    #  * the blend backward stages its rows and gathers them per seed (nesie_blend_conv_backward_staged),
    #    or, for the shapes the tile kernels do not take, sums each seed's taps through an inverted
    #    index (nesie_blend_conv_backward_any; ``blend_backward_form`` chooses);
    #  * group_points / QueryAndGroup / gather_points / three_interpolate backward go through an
    #    inverted index of their indices (``scatter_index``), built on the spot when the caller did
    #    not hand one over (any number of source points);
    # so two runs of the same step give the same bits in every gradient (tests/test_parity_gpu.py).
    DETERMINISTIC = os.environ.get('NESIE_DETERMINISTIC', '1') != '0'

    @classmethod
    def set_deterministic(cls, on=True):
        """Bitwise-reproducible backward (see DETERMINISTIC); -> the previous setting."""
        prev, cls.DETERMINISTIC = cls.DETERMINISTIC, bool(on)
        return prev

    def scatter_index(self, idx, n):
        """(order, sources) = inverted_index(idx, n) when the deterministic backward is on and the
        caller has none, else None (-> the atomic kernels)."""
        if not self.DETERMINISTIC:
            return None
        return self.inverted_index(idx.contiguous(), n)

    def blend_backward_writes_table(self, c, n, segs, m):
        """True when ``blend_conv_backward`` WRITES d_table in full (the staged and the general
        form): the caller then need not zero it."""
        return blend_backward_form(c, n // segs, m, self.DETERMINISTIC) != 'atomic'

    def blend_conv_backward(self, dy, seg_off, idx, weight, rel, d_table, d_wx, segs, seg_len,
                            bn_z=None, bnb=None):
        """dy (B, segs, c, n/segs) -> d_table (B, M, pitch) columns [s*seg_off, +c) and
        sum(dy x rel) WRITTEN to d_wx (segs, c, 3).  bn_z / bnb: dy is the gradient of
        relu(bn(bn_z)) and the norm backward runs on the tile load (bnb (segs*c, 8) from
        ``pw_bnb_coef``).  ``blend_backward_form`` chooses: the staged form and the general form
        (nesie_blend_conv_backward_staged / _any; ``blend_backward_writes_table``) use no float
        atomics, write d_table in full and are bitwise reproducible; the atomic form ADDS its rows
        into d_table (zeroed by the caller)."""
        _check(dy, idx, weight, d_table); _f32(dy, weight, d_table); _i32(idx)
        b, m, pitch = d_table.shape
        n, c = idx.shape[1], dy.shape[2]
        assert tuple(dy.shape) == (b, segs, c, n // segs)
        if d_wx is not None:
            _check(rel, d_wx); _f32(rel, d_wx)
            assert tuple(d_wx.shape) == (segs, c, 3)
        if bnb is not None:
            _check(bn_z, bnb); _f32(bn_z, bnb)
            assert tuple(bn_z.shape) == tuple(dy.shape) and tuple(bnb.shape) == (segs * c, 8)
        form = blend_backward_form(c, n // segs, m, self.DETERMINISTIC)
        if form == 'any':
            self.blend_conv_backward_any(dy, seg_off, idx, weight, rel, d_table, d_wx, segs, seg_len,
                                         bn_z=bn_z, bnb=bnb)
            return
        part = None
        if d_wx is not None:   # one partial per workgroup, summed here
            runs = _lib.load().nesie_blend_conv_runs(n, segs)
            part = torch.empty(b * runs, segs, c, 3, dtype=torch.float32, device=dy.device)
        if form == 'staged':
            assert seg_off == c or segs == 1, 'staged form: one column block per face'
            need = _lib.load().nesie_blend_conv_backward_workspace_bytes(b, c, n, segs)
            ws = torch.empty(need, dtype=torch.uint8, device=dy.device)
            _launch("nesie_blend_conv_backward_staged", dy, b, c, m, n, dy, bn_z, bnb, pitch,
                    seg_off, idx, weight, rel, d_table, part, segs, seg_len, ws, need)
        elif bnb is not None:
            _launch("nesie_blend_conv_backward_bn", dy, b, c, m, n, dy, bn_z, bnb, pitch, seg_off,
                    idx, weight, rel, d_table, part, segs, seg_len)
        else:
            _launch("nesie_blend_conv_backward", dy, b, c, m, n, dy, pitch, seg_off, idx, weight,
                    rel, d_table, part, segs, seg_len)
        if part is not None:      # (d_wx arrives zero-filled or empty from its caller: the sum overwrites it)
            torch.sum(part, 0, out=d_wx)

    def blend_conv_backward_any(self, dy, seg_off, idx, weight, rel, d_table, d_wx, segs, seg_len,
                                bn_z=None, bnb=None):
        """``blend_conv_backward`` by the general form (nesie_blend_conv_backward_any): any c, any
        number of queries per face, any seed count, any pitch; no float atomics, every d_table
        element summed in ascending tap order and written once, d_wx written with the final sum."""
        _check(dy, idx, weight, d_table); _f32(dy, weight, d_table); _i32(idx)
        b, m, pitch = d_table.shape
        n, c = idx.shape[1], dy.shape[2]
        assert tuple(dy.shape) == (b, segs, c, n // segs)
        if pitch != (segs - 1) * seg_off + c or not (seg_off == c or segs == 1):
            d_table.zero_()       # (columns between or behind the faces' blocks: not the kernel's)
        need = _lib.load().nesie_blend_conv_backward_any_workspace_bytes(b, c, m, n, segs)
        ws = _workspace(need, dy.device)
        _launch("nesie_blend_conv_backward_any", dy, b, c, m, n, dy, bn_z, bnb, pitch, seg_off, idx,
                weight, rel, d_table, d_wx, segs, seg_len, ws, need)

    def three_interpolate_grad_wrapper(self, b, c, n, m, grad_out, idx, weight,
                                       grad_points):
        _check(grad_out, idx, weight, grad_points); _f32(grad_out, weight, grad_points)
        _i32(idx)
        assert grad_out.numel() == b * c * n and idx.numel() == b * n * 3
        assert weight.numel() == b * n * 3 and grad_points.numel() == b * c * m
        _launch("nesie_three_interpolate_grad_wrapper", grad_out, b, c, n, m, grad_out, idx, weight,
                grad_points)

    def sort_vertices_forward(self, vertices, mask, num_valid, idx):
        _check(vertices, mask, num_valid, idx); _f32(vertices); _i32(num_valid, idx)
        if mask.dtype != torch.bool:
            raise TypeError("mask must be bool")
        b, n, m, two = vertices.shape
        assert two == 2 and tuple(mask.shape) == (b, n, m)
        assert tuple(num_valid.shape) == (b, n) and tuple(idx.shape) == (b, n, 9)
        _launch("nesie_sort_vertices_forward", vertices, b, n, m, vertices, mask, num_valid, idx)

    def points_in_boxes_batch(self, boxes, pts, out):
        _check(boxes, pts, out); _f32(boxes, pts); _i32(out)
        b, t, seven = boxes.shape
        assert seven == 7 and pts.shape[0] == b and pts.shape[2] == 3
        m = pts.shape[1]
        assert tuple(out.shape) == (b, m, t)
        _launch("nesie_points_in_boxes_batch", boxes, b, t, m, boxes, pts, out)

    def points_in_boxes_gpu(self, boxes, pts, box_idx_of_points):
        """boxes (B,T,7) LiDAR frame, pts (B,M,3) -> box_idx_of_points (B,M) i32: the first box
        that holds the point, else -1; written in full."""
        _check(boxes, pts, box_idx_of_points); _f32(boxes, pts); _i32(box_idx_of_points)
        b, t, seven = boxes.shape
        assert seven == 7 and pts.shape[0] == b and pts.shape[2] == 3
        m = pts.shape[1]
        assert tuple(box_idx_of_points.shape) == (b, m)
        _launch("nesie_points_in_boxes_gpu", boxes, b, t, m, boxes, pts, box_idx_of_points)

    @staticmethod
    def roiaware_pool3d_sizes(n, p, c, out_size, m):
        """-> (elements of pts_idx_of_voxels, of pooled / argmax, of pts_voxel); raises on sizes
        the kernels refuse (nesie_roiaware_pool3d_sizes)."""
        out = (ctypes.c_longlong * 3)()
        _lib.call("nesie_roiaware_pool3d_sizes", n, p, c, *out_size, m, ctypes.addressof(out))
        return tuple(out)

    def roiaware_pool3d_forward(self, rois, pts, pts_feature, argmax, pts_idx_of_voxels,
                                pooled_features, pool_method, pts_voxel=None):
        """rois (N,7), pts (P,3), pts_feature (P,C) -> argmax, pooled_features (N,ox,oy,oz,C),
        pts_idx_of_voxels (N,ox,oy,oz,m) and, when given, the membership table pts_voxel (N,P)
        i32 that ``roiaware_pool3d_backward`` gathers through; all written in full
        (nesie_roiaware_pool3d_forward; pool_method 0 = max, 1 = avg)."""
        _check(rois, pts, pts_feature, argmax, pts_idx_of_voxels, pooled_features)
        _f32(rois, pts, pts_feature, pooled_features); _i32(argmax, pts_idx_of_voxels)
        n, p, c = rois.shape[0], pts.shape[0], pts_feature.shape[1]
        assert tuple(rois.shape) == (n, 7) and tuple(pts.shape) == (p, 3)
        assert tuple(pts_feature.shape) == (p, c)
        assert pts_idx_of_voxels.dim() == 5 and pts_idx_of_voxels.shape[0] == n
        ox, oy, oz, m = (int(s) for s in pts_idx_of_voxels.shape[1:])
        assert tuple(pooled_features.shape) == (n, ox, oy, oz, c)
        assert tuple(argmax.shape) == (n, ox, oy, oz, c)
        assert pool_method in (0, 1)
        if pts_voxel is not None:
            _check(pts_voxel); _i32(pts_voxel)
            assert tuple(pts_voxel.shape) == (n, p)
        _launch("nesie_roiaware_pool3d_forward", rois, n, p, c, m, ox, oy, oz, rois, pts,
                pts_feature, argmax, pts_idx_of_voxels, pooled_features, pts_voxel,
                int(pool_method))

    def roiaware_pool3d_backward(self, pts_idx_of_voxels, argmax, pts_voxel, grad_out, grad_in,
                                 pool_method):
        """grad_out (N,ox,oy,oz,C) -> grad_in (P,C), written in full: every element the sum of its
        contributions in ascending (box, voxel) order (nesie_roiaware_pool3d_backward).  The one
        backward of this op: no float atomics in either setting of ``DETERMINISTIC``."""
        _check(pts_idx_of_voxels, argmax, pts_voxel, grad_out, grad_in)
        _f32(grad_out, grad_in); _i32(pts_idx_of_voxels, argmax, pts_voxel)
        assert grad_out.dim() == 5 and pts_idx_of_voxels.dim() == 5 and pts_voxel.dim() == 2
        n, ox, oy, oz, c = (int(s) for s in grad_out.shape)
        m = int(pts_idx_of_voxels.shape[4])
        p = int(pts_voxel.shape[1])
        assert tuple(pts_idx_of_voxels.shape) == (n, ox, oy, oz, m)
        assert tuple(argmax.shape) == (n, ox, oy, oz, c)
        assert tuple(pts_voxel.shape) == (n, p) and tuple(grad_in.shape) == (p, c)
        assert pool_method in (0, 1)
        _launch("nesie_roiaware_pool3d_backward", grad_out, n, p, ox, oy, oz, c, m,
                pts_idx_of_voxels, argmax, pts_voxel, grad_out, grad_in, int(pool_method))

    @staticmethod
    def voxel_grid_size(voxel_size, coors_range):
        """-> ((grid_x, grid_y, grid_z), cells) of a voxel grid, ``roundf((hi - lo) / vs)`` in fp32;
        raises on a grid the kernels refuse (nesie_voxel_grid_size)."""
        vs = (ctypes.c_float * 3)(*voxel_size)
        cr = (ctypes.c_float * 6)(*coors_range)
        grid, cells = (ctypes.c_int * 3)(), ctypes.c_longlong()
        _lib.call("nesie_voxel_grid_size", ctypes.addressof(vs), ctypes.addressof(cr),
                  ctypes.addressof(grid), ctypes.addressof(cells))
        return tuple(grid), cells.value

    @staticmethod
    def voxel_workspace_bytes(n, cells):
        """Scratch bytes of the sorted voxel ops for n points over ``cells`` cells; raises on sizes
        the kernels refuse (nesie_voxel_workspace_bytes)."""
        out = ctypes.c_longlong()
        _lib.call("nesie_voxel_workspace_bytes", n, cells, ctypes.addressof(out))
        return out.value

    def dynamic_voxelize(self, points, voxel_size, coors_range, coors):
        """points (N,C>=3) -> coors (N,3) i32, (z, y, x) cell or (-1, -1, -1); written in full."""
        _check(points, coors); _f32(points); _i32(coors)
        n, c = points.shape
        assert tuple(coors.shape) == (n, 3)
        vs = (ctypes.c_float * 3)(*voxel_size)
        cr = (ctypes.c_float * 6)(*coors_range)
        _launch("nesie_dynamic_voxelize", points, n, c, points, ctypes.addressof(vs),
                ctypes.addressof(cr), coors)

    def hard_voxelize(self, points, voxel_size, coors_range, voxels, coors, num_points_per_voxel,
                      voxel_num, workspace=None):
        """points (N,C>=3) -> voxels (max_voxels, max_points, C), coors (max_voxels, 3),
        num_points_per_voxel (max_voxels) and voxel_num (1) i32 on the device; only the rows below
        voxel_num are written (nesie_hard_voxelize).  ``workspace`` (uint8, at least
        ``voxel_workspace_bytes``) is allocated when not given."""
        _check(points, voxels, coors, num_points_per_voxel, voxel_num); _f32(points, voxels)
        _i32(coors, num_points_per_voxel, voxel_num)
        n, c = points.shape
        max_voxels, max_points = int(voxels.shape[0]), int(voxels.shape[1])
        assert tuple(voxels.shape) == (max_voxels, max_points, c)
        assert tuple(coors.shape) == (max_voxels, 3)
        assert tuple(num_points_per_voxel.shape) == (max_voxels,) and voxel_num.numel() == 1
        _, cells = self.voxel_grid_size(voxel_size, coors_range)
        need = self.voxel_workspace_bytes(n, cells)
        workspace = self._voxel_workspace(workspace, need, points.device)
        vs = (ctypes.c_float * 3)(*voxel_size)
        cr = (ctypes.c_float * 6)(*coors_range)
        _launch("nesie_hard_voxelize", points, n, c, points, ctypes.addressof(vs),
                ctypes.addressof(cr), max_points, max_voxels, voxels, coors, num_points_per_voxel,
                voxel_num, workspace)

    @staticmethod
    def _voxel_workspace(workspace, need, device):
        if workspace is None:
            return _workspace(need, device)
        _check(workspace)
        if workspace.dtype != torch.uint8 or workspace.numel() < need:
            raise ValueError(f"workspace must be uint8 with at least {need} bytes")
        return workspace

    def dynamic_scatter_forward(self, feats, coors, dims, reduce_type, voxel_feats, voxel_coors,
                                coors_map, reduce_count, num_voxels, order, voxel_start,
                                workspace=None):
        """feats (N,C), coors (N,3) i32, dims 3 exclusive upper bounds, reduce_type 0 sum / 1 mean /
        2 max -> voxel_feats (N,C), voxel_coors (N,3), reduce_count (N) of which the first
        num_voxels (1, on the device) rows are written, coors_map (N) written in full, and order
        (N), voxel_start (N) for the backward (nesie_dynamic_scatter_forward)."""
        _check(feats, coors, voxel_feats, voxel_coors, coors_map, reduce_count, num_voxels, order,
               voxel_start)
        _f32(feats, voxel_feats)
        _i32(coors, voxel_coors, coors_map, reduce_count, num_voxels, order, voxel_start)
        n, c = feats.shape
        assert tuple(coors.shape) == (n, 3) and tuple(voxel_feats.shape) == (n, c)
        assert tuple(voxel_coors.shape) == (n, 3) and num_voxels.numel() == 1
        assert coors_map.numel() == reduce_count.numel() == order.numel() == n
        assert voxel_start.numel() == n and reduce_type in (0, 1, 2)
        d = (ctypes.c_int * 3)(*(int(x) for x in dims))
        cells = d[0] * d[1] * d[2] if min(d) >= 1 else 0
        need = self.voxel_workspace_bytes(n, cells)
        workspace = self._voxel_workspace(workspace, need, feats.device)
        _launch("nesie_dynamic_scatter_forward", feats, n, c, feats, coors, ctypes.addressof(d),
                int(reduce_type), voxel_feats, voxel_coors, coors_map, reduce_count, num_voxels,
                order, voxel_start, workspace)

    def dynamic_scatter_backward(self, grad_voxel, feats, voxel_feats, coors_map, reduce_count,
                                 order, voxel_start, num_voxels, reduce_type, grad_feats):
        """grad_voxel (>=M, C) -> grad_feats (N,C), written in full; a gather, no float atomics
        (nesie_dynamic_scatter_backward)."""
        _check(grad_voxel, feats, voxel_feats, coors_map, reduce_count, order, voxel_start,
               num_voxels, grad_feats)
        _f32(grad_voxel, feats, voxel_feats, grad_feats)
        _i32(coors_map, reduce_count, order, voxel_start, num_voxels)
        n, c = grad_feats.shape
        assert tuple(feats.shape) == (n, c) and coors_map.numel() == n and order.numel() == n
        assert grad_voxel.dim() == 2 and grad_voxel.shape[1] == c and reduce_type in (0, 1, 2)
        _launch("nesie_dynamic_scatter_backward", grad_feats, n, c, grad_voxel, feats, voxel_feats,
                coors_map, reduce_count, order, voxel_start, num_voxels, int(reduce_type),
                grad_feats)

    # ---- sparse 3-D convolution (include/nesie_ops.h, "mmdet3d/ops/spconv")
    @staticmethod
    def _triples(*triples):
        out = []
        for t in triples:
            t = [int(v) for v in t]
            assert len(t) == 3, 'three spatial dimensions only'
            out.append((ctypes.c_int * 3)(*t))
        return out

    @staticmethod
    def spconv_out_shape(spatial_shape, ksize, stride, padding, subm, batch_size):
        """-> ((Do, Ho, Wo), output cells) of a sparse conv; raises on a geometry the kernels
        refuse, a grid of 2^31 cells or more among them (nesie_spconv_out_shape)."""
        sh, ks, st, pd = HipKernels._triples(spatial_shape, ksize, stride, padding)
        out, cells = (ctypes.c_int * 3)(), ctypes.c_longlong()
        _lib.call("nesie_spconv_out_shape", ctypes.addressof(sh), ctypes.addressof(ks),
                  ctypes.addressof(st), ctypes.addressof(pd), int(bool(subm)), int(batch_size),
                  ctypes.addressof(out), ctypes.addressof(cells))
        return tuple(out), cells.value

    @staticmethod
    def spconv_rules_workspace_bytes(n, kvol, subm):
        """Scratch bytes of ``spconv_out_sites``; raises on sizes the sort refuses."""
        out = ctypes.c_longlong()
        _lib.call("nesie_spconv_rules_workspace_bytes", n, int(kvol), int(bool(subm)),
                  ctypes.addressof(out))
        return out.value

    def spconv_out_sites(self, indices, batch_size, spatial_shape, ksize, stride, padding, subm,
                         sorted_keys, sorted_rows, nbr_t, out_indices, counts, workspace=None):
        """Phase 1 of the rulebook: indices (N,4) i32 -> sorted_keys (N), sorted_rows (N),
        nbr_t (N,K) written in full, out_indices (cap,4) rows below M (None for a submanifold conv)
        and counts (2) = {M, offending rows} on the device (nesie_spconv_out_sites)."""
        _check(indices, sorted_keys, sorted_rows, nbr_t, counts)
        _i32(indices, sorted_keys, sorted_rows, nbr_t, counts)
        n = int(indices.shape[0])
        sh, ks, st, pd = self._triples(spatial_shape, ksize, stride, padding)
        kvol = ks[0] * ks[1] * ks[2]
        assert tuple(indices.shape) == (n, 4) and tuple(nbr_t.shape) == (n, kvol)
        assert sorted_keys.numel() == n and sorted_rows.numel() == n and counts.numel() == 2
        if out_indices is not None:
            _check(out_indices); _i32(out_indices)
            _, cells = self.spconv_out_shape(spatial_shape, ksize, stride, padding, subm, batch_size)
            assert out_indices.dim() == 2 and out_indices.shape[1] == 4
            assert out_indices.shape[0] >= min(n * kvol, cells)
        else:
            assert subm, 'a regular conv writes out_indices'
        need = self.spconv_rules_workspace_bytes(n, kvol, subm)
        workspace = self._voxel_workspace(workspace, need, indices.device)
        _launch("nesie_spconv_out_sites", indices, n, indices, int(batch_size),
                ctypes.addressof(sh), ctypes.addressof(ks), ctypes.addressof(st),
                ctypes.addressof(pd), int(bool(subm)), sorted_keys, sorted_rows, nbr_t, out_indices,
                counts, workspace)

    def spconv_gather_table(self, out_indices, sorted_keys, sorted_rows, batch_size, spatial_shape,
                            ksize, stride, padding, subm, nbr, pair_num):
        """Phase 2 of the rulebook: out_indices (M,4) -> nbr (M,K) written in full and pair_num (K)
        (nesie_spconv_gather_table)."""
        _check(out_indices, sorted_keys, sorted_rows, nbr, pair_num)
        _i32(out_indices, sorted_keys, sorted_rows, nbr, pair_num)
        m, n = int(out_indices.shape[0]), int(sorted_keys.numel())
        sh, ks, st, pd = self._triples(spatial_shape, ksize, stride, padding)
        kvol = ks[0] * ks[1] * ks[2]
        assert tuple(out_indices.shape) == (m, 4) and tuple(nbr.shape) == (m, kvol)
        assert sorted_rows.numel() == n and pair_num.numel() == kvol
        _launch("nesie_spconv_gather_table", out_indices, m, out_indices, n, sorted_keys,
                sorted_rows, int(batch_size), ctypes.addressof(sh), ctypes.addressof(ks),
                ctypes.addressof(st), ctypes.addressof(pd), int(bool(subm)), nbr, pair_num)

    def spconv_gather_gemm(self, src, weight, table, dst, weight_transposed=False):
        """dst[r] = sum_k src[table[r, k]] . W[k] (nesie_spconv_gather_gemm): src (S, c_src),
        table (R, K) i32 with entries in -1 .. S - 1, dst (R, c_dst) written in full; weight
        (..., c_src, c_dst) with K leading elements, or (..., c_dst, c_src) read transposed."""
        _check(src, weight, table, dst); _f32(src, weight, dst); _i32(table)
        rows, kvol = (int(s) for s in table.shape)
        c_src, c_dst = int(src.shape[1]), int(dst.shape[1])
        assert src.dim() == 2 and tuple(dst.shape) == (rows, c_dst)
        tail = (c_dst, c_src) if weight_transposed else (c_src, c_dst)
        assert tuple(weight.shape[-2:]) == tail and weight.numel() == kvol * c_src * c_dst
        _launch("nesie_spconv_gather_gemm", dst, rows, int(src.shape[0]), kvol, c_src, c_dst, src,
                weight, bool(weight_transposed), table, dst)

    @staticmethod
    def spconv_wgrad_workspace_bytes(rows, kvol, c_in, c_out):
        out = ctypes.c_longlong()
        _lib.call("nesie_spconv_wgrad_workspace_bytes", rows, int(kvol), int(c_in), int(c_out),
                  ctypes.addressof(out))
        return out.value

    def spconv_wgrad(self, src, dout, table, dw, workspace=None):
        """dw[k] = sum_r src[table[r, k]]^T . dout[r] (nesie_spconv_wgrad): src (S, c_in),
        dout (R, c_out), table (R, K) i32, dw (..., c_in, c_out) with K leading elements, written
        in full in a fixed order."""
        _check(src, dout, table, dw); _f32(src, dout, dw); _i32(table)
        rows, kvol = (int(s) for s in table.shape)
        c_in, c_out = int(src.shape[1]), int(dout.shape[1])
        assert src.dim() == 2 and tuple(dout.shape) == (rows, c_out)
        assert tuple(dw.shape[-2:]) == (c_in, c_out) and dw.numel() == kvol * c_in * c_out
        assert rows > 0 and src.shape[0] > 0, 'an empty product is zeros: the caller writes them'
        need = self.spconv_wgrad_workspace_bytes(rows, kvol, c_in, c_out)
        workspace = self._voxel_workspace(workspace, need, src.device)
        _launch("nesie_spconv_wgrad", dw, rows, int(src.shape[0]), kvol, c_in, c_out, src, dout,
                table, dw, workspace)

    def vote_targets(self, points, gt_boxes, gt_count):
        """points (B,N,C>=3), depth-frame gt_boxes (B,T,7), gt_count (B) int64 -> vote targets
        (B,N,9) and masks (B,N) int64 of get_targets_single, one launch."""
        _check(points, gt_boxes, gt_count); _f32(points, gt_boxes)
        b, n, c = points.shape
        t = gt_boxes.shape[1]
        assert gt_boxes.shape == (b, t, 7) and gt_count.shape == (b,) and gt_count.dtype == torch.int64
        votes = points.new_empty(b, n, 9)
        masks = torch.empty(b, n, dtype=torch.int64, device=points.device)
        _launch("nesie_vote_targets", points, b, t, n, c, gt_boxes if t else None, gt_count, points,
                votes, masks)
        return votes, masks

    def group_max_pool_forward(self, x, out, argmax):
        """x (..., ns) -> out (...), argmax (...) uint8."""
        _check(x, out, argmax); _f32(x, out)
        ns = x.shape[-1]
        rows = x.numel() // ns
        assert out.numel() == rows and argmax.numel() == rows and argmax.dtype == torch.uint8
        _launch("nesie_group_max_pool_forward", x, rows, ns, x, out, argmax)

    def group_max_pool_backward(self, grad_out, argmax, grad_x):
        _check(grad_out, argmax, grad_x); _f32(grad_out, grad_x)
        ns = grad_x.shape[-1]
        rows = grad_x.numel() // ns
        assert grad_out.numel() == rows and argmax.numel() == rows
        _launch("nesie_group_max_pool_backward", grad_x, rows, ns, grad_out, argmax, grad_x)


    def group_max_pool_backward_add(self, grad_out, argmax, grad_x):
        """grad_x[..., argmax] += grad_out, in place (grad_x (..., ns) contiguous)."""
        _check(grad_out, argmax, grad_x); _f32(grad_out, grad_x)
        ns = grad_x.shape[-1]
        rows = grad_x.numel() // ns
        assert grad_out.numel() == rows and argmax.numel() == rows
        _launch("nesie_group_max_pool_backward_add", grad_x, rows, ns, grad_out, argmax, grad_x)

    def channel_sum(self, x, out=None, ng=1):
        """x (NB, C, P) (batch stride free, each x[n] (C, P) contiguous) -> (ng * C,) sums over the
        batch entries n = g (mod ng) and the positions, in a fixed order (nesie_channel_sum): a conv
        bias's gradient (ng > 1: S stacked nets whose batch axis runs (scene, net))."""
        _f32(x)
        nb, c, p = x.shape
        assert x.is_cuda and x.stride(2) == 1 and x.stride(1) == p and nb % ng == 0
        if out is None:
            out = torch.empty(ng * c, dtype=torch.float32, device=x.device)
        _check(out); _f32(out)
        assert out.numel() == ng * c
        _launch("nesie_channel_sum", x, nb, ng, c, p, x, x.stride(0) if nb > 1 else c * p, out)
        return out

    def lhs_nms_samecls(self, boxes, thr, keep):
        """boxes (B,K,8) f32, keep (B,K) uint8."""
        _check(boxes, keep); _f32(boxes)
        b, k, eight = boxes.shape
        assert eight == 8 and tuple(keep.shape) == (b, k) and keep.dtype == torch.uint8
        _launch("nesie_lhs_nms_samecls", boxes, b, k, boxes, float(thr), keep)

    def iou3d_forward(self, box1, box2, iou, jac):
        """box1, box2 (n,7); iou (n,); jac (n,7) or None."""
        _check(box1, box2, iou); _f32(box1, box2, iou)
        n = iou.numel()
        assert box1.numel() == n * 7 and box2.numel() == n * 7
        if jac is not None:
            _check(jac); _f32(jac)
            assert jac.numel() == n * 7
        _launch("nesie_iou3d_forward", box1, n, box1, box2, iou, jac)

    def giou3d_forward(self, box1, box2, kind, enclosing, loss, iou, jac):
        """box1, box2 (n,7); kind 0 GIoU / 1 DIoU; enclosing 0 smallest / 1 aligned; loss (n,);
        iou (n,) or None; jac (n,7) = d loss / d box1, or None (nesie_giou3d_forward)."""
        _check(box1, box2, loss); _f32(box1, box2, loss)
        n = loss.numel()
        assert box1.numel() == n * 7 and box2.numel() == n * 7
        if iou is not None:
            _check(iou); _f32(iou)
            assert iou.numel() == n
        if jac is not None:
            _check(jac); _f32(jac)
            assert jac.numel() == n * 7
        _launch("nesie_giou3d_forward", box1, n, box1, box2, int(kind), int(enclosing), loss, iou,
                jac)

    @staticmethod
    def _aa_rows(count, *named):
        """Each (name, tensor or None, rows) of an axis-aligned IoU launch: a device f32 tensor of
        rows x 6 whose rows can be read as 8-byte pairs."""
        for name, t, rows in named:
            if t is None:
                continue
            _check(t); _f32(t)
            assert t.numel() == count * rows * 6, (name, tuple(t.shape), count, rows)
            assert t.data_ptr() % 8 == 0, f'{name}: rows must be 8-byte aligned'

    def aa_iou3d_paired_forward(self, box1, box2, mode, eps, out, jac1=None, jac2=None):
        """box1, box2 (n,6) corners; mode 0 IoU / 1 GIoU; out (n,); jac1, jac2 (n,6) = d out / d box1,
        d out / d box2, or None (nesie_aa_iou3d_paired_forward)."""
        _check(out); _f32(out)
        n = out.numel()
        self._aa_rows(1, ('box1', box1, n), ('box2', box2, n), ('jac1', jac1, n), ('jac2', jac2, n))
        _launch("nesie_aa_iou3d_paired_forward", box1, n, box1, box2, int(mode), float(eps), out,
                jac1, jac2)

    def aa_iou3d_matrix_forward(self, box1, box2, mode, eps, out):
        """box1 (b,m,6), box2 (b,n,6) corners; out (b,m,n) (nesie_aa_iou3d_matrix_forward)."""
        _check(out); _f32(out)
        b, m, n = out.shape
        self._aa_rows(b, ('box1', box1, m), ('box2', box2, n))
        _launch("nesie_aa_iou3d_matrix_forward", box1, b, m, n, box1, box2, int(mode), float(eps),
                out)

    def aa_iou3d_matrix_backward(self, box1, box2, mode, eps, grad_out, grad1=None, grad2=None):
        """grad_out (b,m,n) -> grad1 (b,m,6) and / or grad2 (b,n,6), in a fixed summation order
        (nesie_aa_iou3d_matrix_backward)."""
        _check(grad_out); _f32(grad_out)
        b, m, n = grad_out.shape
        self._aa_rows(b, ('box1', box1, m), ('box2', box2, n), ('grad1', grad1, m),
                      ('grad2', grad2, n))
        _launch("nesie_aa_iou3d_matrix_backward", box1, b, m, n, box1, box2, int(mode), float(eps),
                grad_out, grad1, grad2)

    def conv_wgrad(self, dy, x, dw, x_coef=None, x_relu=False, bn_z=None, bnb=None):
        """dw (cout, cin) = sum_b dy[b] (cout, P) @ act(x[b]) (cin, P)^T on the matrix cores;
        dy and x may be batch-strided views (each dy[b], x[b] contiguous).  bn_z / bnb: dy is the
        gradient of relu(bn(bn_z)) and the norm backward runs on the load (nesie_conv_wgrad_bn)."""
        _f32(dy, x, dw)
        if not (dy.is_cuda and dw.is_contiguous()):
            raise ValueError("conv_wgrad: HIP tensors, dw contiguous")
        b, cout, p = dy.shape
        cin = x.shape[1]
        assert x.shape[0] == b and x.shape[2] == p and tuple(dw.shape) == (cout, cin)
        assert x.stride(2) == 1 and x.stride(1) == p, "each x[b] must be (cin, P) contiguous"
        assert dy.stride(2) == 1 and dy.stride(1) == p, "each dy[b] must be (cout, P) contiguous"
        lib = _lib.load()
        need = lib.nesie_conv_wgrad_workspace_bytes(b, cout, cin, p)
        ws = _workspace(need, dy.device)
        if bnb is not None:
            _check(bn_z, bnb); _f32(bn_z, bnb)
            assert tuple(bn_z.shape) == tuple(dy.shape) and dy.is_contiguous() and tuple(bnb.shape) == (cout, 8)
            _launch("nesie_conv_wgrad_bn", dy, b, cout, cin, p, dy, bn_z, cout * p, bnb, x,
                    x.stride(0) if b > 1 else cin * p, x_coef, bool(x_relu), dw, ws, need)
            return
        _launch("nesie_conv_wgrad", dy, b, cout, cin, p, dy, dy.stride(0) if b > 1 else cout * p, x,
                x.stride(0) if b > 1 else cin * p, x_coef, bool(x_relu), dw, ws, need)

    def pw_wgrad_supported(self, co, ci, p):
        return bool(_lib.load().nesie_pw_wgrad_supported(int(co), int(ci), int(p)))

    def pw_wgrad_tiled(self, nb, ng, co, ci, p):
        """True when ``pw_wgrad`` serves this shape as ONE launch over 64 x 64 blocks of the product
        (wide layers over few positions: the 1-D chains)."""
        return bool(_lib.load().nesie_pw_wgrad_tiled(int(nb), int(ng), int(co), int(ci), int(p)))

    # ---- deferred weight-gradient reductions ("Deferred reductions", include/nesie_ops.h) -------
    # Between ``begin_deferred_reductions()`` and ``flush_deferred_reductions()`` a weight gradient
    # whose destination is FINAL (a slot of the flat gradient vector: nothing reads it before the
    # optimiser) leaves the addition of its partials pending; the flush runs them all in one launch.
    # dp.FlatTrainState opens the window in begin() and flushes in collect().  NESIE_DEFER_WGRAD=0:
    # every reduction runs with its own launch (A/B switch).
    DEFER_WGRAD = os.environ.get('NESIE_DEFER_WGRAD', '1') != '0'
    _deferred = None       # None: no window open; else the workspaces (and destinations) kept alive

    @classmethod
    def begin_deferred_reductions(cls):
        if cls._deferred:      # a window left open by an aborted backward: its partials are stale
            _lib.call("nesie_pw_wgrad_drop_deferred")
        cls._deferred = [] if cls.DEFER_WGRAD else None

    @classmethod
    def flush_deferred_reductions(cls, device=None, close=False):
        """Finish every pending weight gradient (one launch on the current stream); -> the
        destinations that were written.  ``close``: end the window."""
        held, done = cls._deferred, []
        if held:
            dev = device if device is not None else held[0][1].device
            _launch("nesie_pw_wgrad_flush_deferred", torch.device(dev))
            done = [dw for _, dw in held]
            # (under a graph capture the workspaces live in the graph's pool; in eager mode the caching
            # allocator hands a freed block to later launches of this stream only: both orders are safe)
            cls._deferred = []
        if close:
            cls._deferred = None
        return done

    @staticmethod
    def _wgrad_scratch(nb, ng, co, ci, p, dw, final):
        """Scratch of one weight-gradient launch into ``dw`` -> (workspace, its bytes, defer).
        defer: ``final`` and a window is open; (workspace, dw) is then held BEFORE the launch, so that
        a launch that raises after the library queued its reduction still leaves a non-empty list and
        the next ``begin_deferred_reductions()`` drops the queue (which points at this workspace)."""
        need = _lib.load().nesie_pw_wgrad_workspace_bytes(nb, ng, co, ci, p)
        ws = _workspace(need, dw.device)
        defer = bool(final) and HipKernels._deferred is not None
        if defer:
            HipKernels._deferred.append((ws, dw))
        return ws, need, defer

    def pw_wgrad(self, dy, x, dw, ng=1, x_coef=None, x_relu=True, final=False):
        """dw (ng, co, ci) = sum over n % ng == g and positions of dy[n] (co, P) act(x[n])^T
        (nesie_pw_wgrad); dy (NB, co, P), x (NB, ci, P) batch-strided views allowed;
        x_coef (ng*ci, 4) folded BatchNorm of x.  ``final``: dw is read by nobody before the
        deferred reductions are flushed (a slot of the flat gradient vector)."""
        _f32(dy, x, dw)
        nb, co, p = dy.shape
        ci = x.shape[1]
        assert dy.is_cuda and x.shape[0] == nb and x.shape[2] == p and nb % ng == 0
        assert dw.is_contiguous() and dw.numel() == ng * co * ci
        assert x.stride(2) == 1 and x.stride(1) == p and dy.stride(2) == 1 and dy.stride(1) == p
        if x_coef is not None:
            _check(x_coef); _f32(x_coef)
            assert tuple(x_coef.shape) == (ng * ci, 4)
        ws, need, defer = self._wgrad_scratch(nb, ng, co, ci, p, dw, final)
        _launch("nesie_pw_wgrad", dy, nb, ng, co, ci, p, dy, dy.stride(0) if nb > 1 else co * p, x,
                x.stride(0) if nb > 1 else ci * p, x_coef, bool(x_relu), dw, ws, need, defer)

    def pw_bnb_coef(self, part, z_coef, gamma, count, dgamma, dbeta):
        """(channels, 8) reduction coefficients of a BatchNorm + ReLU backward from the partial sums
        part (channels, slots, 2) of ``pw_dgrad_bn_reduce`` (nesie_pw_bnb_coef); writes dgamma, dbeta."""
        _check(part, z_coef, dgamma, dbeta); _f32(part, z_coef, dgamma, dbeta)
        ch = part.shape[0]
        assert part.dim() == 3 and part.shape[2] == 2 and tuple(z_coef.shape) == (ch, 4)
        assert dgamma.numel() == ch == dbeta.numel()
        if gamma is not None:
            _check(gamma); _f32(gamma)
        bnb = torch.empty(ch, 8, dtype=torch.float32, device=part.device)
        _launch("nesie_pw_bnb_coef", part, ch, part.shape[1], float(count), part, z_coef, gamma,
                bnb, dgamma, dbeta)
        return bnb

    def pw_wgrad_bn_supported(self, co, ci, p):
        return bool(_lib.load().nesie_pw_wgrad_bn_supported(int(co), int(ci), int(p)))

    def pw_wgrad_bn_backward(self, da, z, z_coef, gamma, part, x, dz, dw, dgamma, dbeta, ng=1,
                             x_coef=None, x_relu=True, d_row_bias=None, group=0, final=False):
        """The BatchNorm + ReLU backward's apply pass fused into the weight gradient it feeds
        (nesie_pw_wgrad_bn_backward): da (NB, co, P) gradient of relu(bn(z)), z raw conv output,
        z_coef (ng*co, 4), part (ng*co, slots, 2) from ``pw_dgrad_bn_reduce``; x (NB, ci, P) the
        layer's input with its own folded norm x_coef.  Writes dz (may be da), dw (ng, co, ci),
        dgamma, dbeta (ng*co); d_row_bias (NB, co, P / group), group 16 or 64: the gradient of the
        per-group row bias the forward added to z (zero-filled by the caller for group 64)."""
        _f32(da, z, x, dz, dw, dgamma, dbeta); _check(z_coef, part, dz); _f32(z_coef, part)
        nb, co, p = da.shape
        ci = x.shape[1]
        assert da.is_cuda and tuple(z.shape) == (nb, co, p) == tuple(dz.shape) and x.shape[0] == nb
        assert x.shape[2] == p and nb % ng == 0 and da.is_contiguous() and z.is_contiguous()
        assert dw.is_contiguous() and dw.numel() == ng * co * ci
        assert x.stride(2) == 1 and x.stride(1) == p
        assert tuple(z_coef.shape) == (ng * co, 4) and part.dim() == 3 and part.shape[0] == ng * co
        assert dgamma.numel() == ng * co == dbeta.numel()
        if d_row_bias is not None:
            _check(d_row_bias); _f32(d_row_bias)
            assert group in (16, 64) and d_row_bias.numel() == nb * co * (p // group)
        if gamma is not None:
            _check(gamma); _f32(gamma)
        if x_coef is not None:
            _check(x_coef); _f32(x_coef)
            assert tuple(x_coef.shape) == (ng * ci, 4)
        ws, need, defer = self._wgrad_scratch(nb, ng, co, ci, p, dw, final)
        cws = torch.empty(ng * co, 8, dtype=torch.float32, device=da.device)
        _launch("nesie_pw_wgrad_bn_backward", da, nb, ng, co, ci, p, da, z, co * p, z_coef, gamma,
                part, part.shape[1], x, x.stride(0) if nb > 1 else ci * p, x_coef, bool(x_relu), dz,
                dw, dgamma, dbeta, cws, d_row_bias, int(group), ws, need, defer)

    @staticmethod
    def conv_wgrad_supported(cout, cin):
        return (cout <= 128 and cin <= 288) or (cout <= 256 and cin <= 128)

    @staticmethod
    def _bn_pool_ws(x):
        b, c, m, ns = x.shape
        need = _lib.load().nesie_bn_workspace_bytes(b, c, m * ns)
        return _workspace(need, x.device), need

    def bn_relu_maxpool_forward(self, x, gamma, beta, running_mean, running_var, momentum, eps,
                                pooled, argmax, save_mean, save_invstd, fwd_coef):
        """x (B, C, M, ns) -> pooled (B, C, M) fp32, argmax (B, C, M) uint8."""
        _check(x, pooled, argmax, save_mean, save_invstd, fwd_coef); _f32(x, pooled)
        b, c, m, ns = x.shape
        assert tuple(pooled.shape) == (b, c, m) and argmax.dtype == torch.uint8
        ws, need = self._bn_pool_ws(x)
        _launch("nesie_bn_relu_maxpool_forward", x, b, c, m, ns, x, gamma, beta, running_mean,
                running_var, float(momentum), float(eps), pooled, argmax, save_mean, save_invstd,
                fwd_coef, ws, need)

    def bn_relu_maxpool_backward(self, grad_pooled, argmax, x, pooled, gamma, save_invstd,
                                 fwd_coef, dx, dgamma, dbeta):
        _check(grad_pooled, argmax, x, pooled, dx); _f32(grad_pooled, x, pooled, dx)
        b, c, m, ns = x.shape
        assert tuple(grad_pooled.shape) == (b, c, m) and dx.shape == x.shape
        ws, need = self._bn_pool_ws(x)
        _launch("nesie_bn_relu_maxpool_backward", x, b, c, m, ns, grad_pooled, argmax, x, pooled,
                gamma, save_invstd, fwd_coef, dx, dgamma, dbeta, ws, need)

    def bn_relu_forward(self, x, gamma, beta, running_mean, running_var, momentum, eps, relu,
                        y, save_mean, save_invstd, fwd_coef, row_bias=None, pre_partial=None):
        """x, y (B, C, *) fp32; per-channel vectors [C]; running stats updated in place.
        row_bias (B, C, K): added to x broadcast over the last axis of x (B, C, K, G)."""
        _check(x, y, save_mean, save_invstd); _f32(x, y, save_mean, save_invstd)
        b, c = x.shape[:2]
        p = x.numel() // (b * c) if b * c else 0
        group = _row_bias_group(x, row_bias)
        need = _lib.load().nesie_bn_workspace_bytes(b, c, p)
        ws = _workspace(need, x.device)
        _launch("nesie_bn_relu_forward", x, b, c, p, x, gamma, beta, running_mean, running_var,
                float(momentum), float(eps), bool(relu), y, save_mean, save_invstd, fwd_coef,
                row_bias, group, pre_partial,
                0 if pre_partial is None else pre_partial.numel() // (2 * c), ws, need)

    def pw_supported(self, k, cout, p):
        return bool(_lib.load().nesie_pw_supported(int(k), int(cout), int(p)))

    def pw_stat_slots(self, nb, ng, k, cout, p):
        return int(_lib.load().nesie_pw_stat_slots(nb, ng, k, cout, p))

    def pw_layer_forward(self, x, w, ng=1, in_coef=None, in_relu=True, row_bias=None, rb_group=0,
                         bias=None, y=None, stat_part=None, pool_group=0, pool_min=False,
                         pool_out=None):
        """y[n] = W[n % ng] . act(x[n]) (+ row_bias) (+ bias) on the matrix cores
        (nesie_pw_layer_forward).  x (NB, K, P) with each x[n] contiguous (batch stride free);
        w (ng, Cout, K) as ANY strided view (a transposed view gives the input-gradient product);
        in_coef (ng*K, 4) folded BatchNorm of the operand; y (NB, Cout, P) or None;
        stat_part (ng, slots, Cout, 4); pool_out = (max, min | None, argmax, argmin | None), each
        (NB, Cout, P / pool_group)."""
        _f32(x, w)
        nb, k, p = x.shape
        assert w.dim() == 3 and w.shape[0] == ng and w.shape[2] == k and nb % ng == 0
        cout = w.shape[1]
        assert x.is_cuda and x.stride(2) == 1 and x.stride(1) == p, "each x[n] must be (K, P) contiguous"
        if y is not None:
            _f32(y)
            assert y.is_cuda and tuple(y.shape) == (nb, cout, p) and y.stride(2) == 1 \
                and y.stride(1) == p, "each y[n] must be (Cout, P) contiguous"
        if stat_part is not None:
            _check(stat_part); _f32(stat_part)
            assert tuple(stat_part.shape) == (ng, self.pw_stat_slots(nb, ng, k, cout, p), cout, 4)
        if in_coef is not None:
            _check(in_coef); _f32(in_coef)
            assert tuple(in_coef.shape) == (ng * k, 4)
        if row_bias is not None:
            _check(row_bias); _f32(row_bias)
            assert row_bias.numel() == nb * cout * (p // rb_group)
        if bias is not None:
            _check(bias); _f32(bias)
            assert bias.numel() == ng * cout
        pmax = pmin = amax = amin = None
        if pool_group:
            pmax, pmin, amax, amin = pool_out
            for t in (pmax, pmin):
                if t is not None:
                    _check(t); _f32(t)
                    assert t.numel() == nb * cout * (p // pool_group)
            for t in (amax, amin):
                if t is not None:
                    _check(t)
                    assert t.dtype == torch.uint8 and t.numel() == nb * cout * (p // pool_group)
            assert (pmin is not None) == bool(pool_min)
        _launch("nesie_pw_layer_forward", x, nb, ng, k, cout, p, x,
                x.stride(0) if nb > 1 else k * p, w, w.stride(0) if ng > 1 else 0, w.stride(1),
                w.stride(2), in_coef, bool(in_relu), row_bias, int(rb_group), bias, y,
                y.stride(0) if (y is not None and nb > 1) else cout * p, stat_part, int(pool_group),
                bool(pool_min), pmax, pmin, amax, amin)

    # ---- SA1's first layer without its output tensor (include/nesie_ops.h, "round 5: the first
    # shared-MLP layer ... WITHOUT its output tensor")
    @staticmethod
    def _k4_check(x4, w0):
        _f32(x4, w0); _check(w0)
        nb, c, p = x4.shape
        assert x4.is_cuda and c == 4 and x4.stride(2) == 1 and x4.stride(1) == p and tuple(w0.shape) == (64, 4)
        return nb, p

    def k4_supported(self, c0, c1, c2, p):
        """SA1's shape: 4 -> 64 -> 64 over whole 64-position tiles."""
        return c0 == 4 and c1 == 64 and c2 == 64 and p % 64 == 0 and self.pw_supported(64, 64, p) \
            and self.pw_wgrad_bn_supported(64, 64, p)

    def pw_layer_forward_k4(self, x4, w0, w, in_coef, y, stat_part):
        """y[n] = W . relu(bn(W0 . x4[n])) with the inner 64-row tensor rebuilt in the staging
        (nesie_pw_layer_forward_k4): x4 (NB, 4, P), w0 (64, 4), w (Cout = 64, 64) any strided view,
        in_coef (64, 4) the first layer's folded norm, y (NB, 64, P), stat_part as pw_layer_forward."""
        nb, p = self._k4_check(x4, w0)
        _f32(w, y); _check(in_coef, y, stat_part); _f32(in_coef, stat_part)
        cout = w.shape[0]
        assert tuple(w.shape) == (cout, 64) and tuple(y.shape) == (nb, cout, p) and tuple(in_coef.shape) == (64, 4)
        assert tuple(stat_part.shape) == (1, self.pw_stat_slots(nb, 1, 64, cout, p), cout, 4)
        _launch("nesie_pw_layer_forward_k4", x4, nb, cout, p, x4, x4.stride(0) if nb > 1 else 4 * p,
                w0, w, w.stride(0), w.stride(1), in_coef, y, cout * p, stat_part)

    def pw_dgrad_bn_reduce_k4(self, dy, w, x4, w0, z_coef):
        """The reductions of ``pw_dgrad_bn_reduce`` for a layer whose input was relu(bn(W0 . x4)),
        WITHOUT the input gradient itself (nesie_pw_dgrad_bn_reduce_k4): dy (NB, K, P), w the
        transposed weight view (64, K) -> (part (64, slots, 2), g_part (64, slots, 4))."""
        nb, p = self._k4_check(x4, w0)
        _f32(dy, w); _check(z_coef); _f32(z_coef)
        k = dy.shape[1]
        assert tuple(dy.shape) == (nb, k, p) and dy.is_cuda and dy.stride(2) == 1 and dy.stride(1) == p
        assert tuple(w.shape) == (64, k) and tuple(z_coef.shape) == (64, 4)
        slots = self.pw_stat_slots(nb, 1, k, 64, p)
        part = torch.empty(64, slots, 2, dtype=torch.float32, device=dy.device)
        g_part = torch.empty(64, slots, 4, dtype=torch.float32, device=dy.device)
        _launch("nesie_pw_dgrad_bn_reduce_k4", dy, nb, k, p, dy, dy.stride(0) if nb > 1 else k * p,
                w, w.stride(0), w.stride(1), x4, x4.stride(0) if nb > 1 else 4 * p, w0, z_coef,
                part, g_part)
        return part, g_part

    def pw_wgrad_bn_backward_k4(self, da, z, z_coef, gamma, part, x4, w0, x_coef, dw, dgamma, dbeta,
                                final=False):
        """``pw_wgrad_bn_backward`` of a 64 x 64 layer whose X operand is relu(bn(W0 . x4)), rebuilt on
        the load (nesie_pw_wgrad_bn_backward_k4); dz is written over da."""
        nb, p = self._k4_check(x4, w0)
        _f32(da, z, dw, dgamma, dbeta); _check(da, z, z_coef, part, x_coef, dw); _f32(z_coef, part, x_coef)
        assert tuple(da.shape) == (nb, 64, p) == tuple(z.shape) and dw.numel() == 64 * 64
        assert tuple(z_coef.shape) == (64, 4) == tuple(x_coef.shape) and part.shape[0] == 64 and part.shape[2] == 2
        if gamma is not None:
            _check(gamma); _f32(gamma)
        ws, need, defer = self._wgrad_scratch(nb, 1, 64, 64, p, dw, final)
        cws = torch.empty(64, 8, dtype=torch.float32, device=da.device)
        _launch("nesie_pw_wgrad_bn_backward_k4", da, nb, p, da, z, 64 * p, z_coef, gamma, part,
                part.shape[1], x4, x4.stride(0) if nb > 1 else 4 * p, w0, x_coef, da, dw, dgamma,
                dbeta, cws, ws, need, defer)

    def pw_wgrad_bn_backward_k4_fused(self, da, z, z_coef, gamma, part, x4, w0, x_coef, w, dw, dgamma, dbeta,
                                      final=False):
        """``pw_wgrad_bn_backward_k4`` + ``pw_dgrad_bn_reduce_k4`` as one launch
        (nesie_pw_wgrad_bn_backward_k4_fused): w (64, 64) the layer's weight; da is NOT overwritten (dz is
        consumed inside the launch).  -> (in_part (64, slots, 2), in_gpart (64, slots, 4))."""
        nb, p = self._k4_check(x4, w0)
        _f32(da, z, dw, dgamma, dbeta, w); _check(da, z, z_coef, part, x_coef, dw, w); _f32(z_coef, part, x_coef)
        assert tuple(da.shape) == (nb, 64, p) == tuple(z.shape) and dw.numel() == 64 * 64 and tuple(w.shape) == (64, 64)
        assert tuple(z_coef.shape) == (64, 4) == tuple(x_coef.shape) and part.shape[0] == 64 and part.shape[2] == 2
        if gamma is not None:
            _check(gamma); _f32(gamma)
        slots = _lib.load().nesie_pw_wgrad_bn_backward_k4_slots(nb, p)
        ws, need, defer = self._wgrad_scratch(nb, 1, 64, 64, p, dw, final)
        cws = torch.empty(64, 8, dtype=torch.float32, device=da.device)
        in_part = torch.empty(64, slots, 2, dtype=torch.float32, device=da.device)
        in_gpart = torch.empty(64, slots, 4, dtype=torch.float32, device=da.device)
        _launch("nesie_pw_wgrad_bn_backward_k4_fused", da, nb, p, da, z, 64 * p, z_coef, gamma,
                part, part.shape[1], x4, x4.stride(0) if nb > 1 else 4 * p, w0, x_coef, w, dw,
                dgamma, dbeta, cws, in_part, in_gpart, ws, need, defer)
        return in_part, in_gpart

    def k4_moments(self, x4):
        """-> (256, 20) float64 per-workgroup partial sums of X4[j] and X4[j] X4[k] (nesie_k4_moments)."""
        _f32(x4)
        nb, c, p = x4.shape
        assert x4.is_cuda and c == 4 and x4.stride(2) == 1 and x4.stride(1) == p
        need = _lib.load().nesie_k4_moments_bytes()
        mom = torch.empty(need // 160, 20, dtype=torch.float64, device=x4.device)
        _launch("nesie_k4_moments", x4, nb, p, x4, x4.stride(0) if nb > 1 else 4 * p, mom)
        return mom

    def k4_stat_finalize(self, mom, w0, gamma, beta, running_mean, running_var, momentum, eps, count, coef):
        """Training-mode BatchNorm coefficients of W0 . X4 from the moments of X4 (nesie_k4_stat_finalize)."""
        _check(mom, w0, coef); _f32(w0, coef)
        assert mom.dtype == torch.float64 and tuple(w0.shape) == (64, 4) and tuple(coef.shape) == (64, 4)
        _launch("nesie_k4_stat_finalize", mom, float(count), mom, w0, gamma, beta, running_mean,
                running_var, float(momentum), float(eps), coef)

    def k4_first_layer_wgrad(self, mom, w0, bnb, g_part, dw):
        """dW0 (64, 4) from the reductions (nesie_k4_first_layer_wgrad): mom from ``k4_moments``, bnb (64, 8)
        from ``pw_bnb_coef`` over the part of ``pw_dgrad_bn_reduce_k4``, g_part (64, slots, 4) of the same."""
        _check(mom, w0, bnb, g_part, dw); _f32(w0, bnb, g_part, dw)
        assert mom.dtype == torch.float64 and tuple(w0.shape) == (64, 4)
        assert tuple(bnb.shape) == (64, 8) and g_part.shape[0] == 64 and g_part.shape[2] == 4 and dw.numel() == 256
        _launch("nesie_k4_first_layer_wgrad", mom, mom, w0, bnb, g_part, g_part.shape[1], dw)

    def pw_dgrad_bn_reduce(self, dy, w, z, z_coef, da, ng=1):
        """da[n] = W[n % ng] . dy[n] (w = the transposed weight view (ng, Cin, Cout)) plus the
        reduction of the backward of relu(bn(z)) that consumes da (nesie_pw_dgrad_bn_reduce):
        -> partials (ng*Cin, slots, 2) for ``bn_relu_backward_apply``.  z (NB, Cin, P) raw conv
        output, z_coef (ng*Cin, 4) its folded BatchNorm."""
        _f32(dy, w, z, da); _check(z_coef); _f32(z_coef)
        nb, k, p = dy.shape
        cout = w.shape[1]
        assert w.dim() == 3 and w.shape[0] == ng and w.shape[2] == k and nb % ng == 0
        for t in (dy, z, da):
            assert t.is_cuda and t.stride(2) == 1 and t.stride(1) == p
        assert tuple(z.shape) == (nb, cout, p) == tuple(da.shape) and tuple(z_coef.shape) == (ng * cout, 4)
        part = torch.empty(ng * cout, self.pw_stat_slots(nb, ng, k, cout, p), 2,
                           dtype=torch.float32, device=dy.device)
        bs = lambda t, rows: t.stride(0) if nb > 1 else rows * p  # noqa: E731
        _launch("nesie_pw_dgrad_bn_reduce", dy, nb, ng, k, cout, p, dy, bs(dy, k), w,
                w.stride(0) if ng > 1 else 0, w.stride(1), w.stride(2), da, bs(da, cout), z,
                bs(z, cout), z_coef, part)
        return part

    def bn_relu_backward_apply(self, dy, x, gamma, save_invstd, fwd_coef, partial, dx, dgamma,
                               dbeta, d_row_bias=None, group=None):
        """Apply pass of the BatchNorm + ReLU backward from ready partials (C, nslice, 2); x is
        the raw conv output of the fused forward (nesie_bn_relu_backward_apply).  save_invstd None:
        column 3 of fwd_coef."""
        _check(dy, x, dx, fwd_coef, partial); _f32(dy, x, dx, partial)
        b, c = x.shape[:2]
        p = x.numel() // (b * c) if b * c else 0
        assert partial.dim() == 3 and partial.shape[0] == c and partial.shape[2] == 2
        if d_row_bias is not None:
            _check(d_row_bias); _f32(d_row_bias)
            assert group and d_row_bias.numel() == b * c * (p // group)
        _launch("nesie_bn_relu_backward_apply", x, b, c, p, dy, x, gamma, save_invstd, fwd_coef,
                partial, int(partial.shape[1]), dx, dgamma, dbeta, int(group or 1), d_row_bias)

    def vote_loss_forward(self, seed, vote, seed_idx, mask, targets, w_dst, ticket):
        """-> (loss scalar, sign (B,N,3), scale scalar) (nesie_vote_loss_forward)."""
        _check(seed, vote, seed_idx, mask, targets); _f32(seed, vote, targets)
        assert seed_idx.dtype == torch.int64 and mask.dtype == torch.int64
        b, n = seed.shape[:2]
        npts = mask.shape[1]
        gps = targets.shape[2] // 3
        assert tuple(vote.shape) == (b, n, 3) and tuple(targets.shape) == (b, npts, 3 * gps)
        dev = seed.device
        sign = torch.empty(b, n, 3, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        scale = torch.empty((), dtype=torch.float32, device=dev)
        partial = torch.empty(64, 2, dtype=torch.float32, device=dev)
        _launch("nesie_vote_loss_forward", seed, b, n, npts, gps, seed, vote, seed_idx, mask,
                targets, float(w_dst), sign, loss, scale, partial, ticket)
        return loss, sign, scale

    def vote_loss_backward(self, g, scale, sign):
        _check(g, scale, sign); _f32(g, scale, sign)
        d = torch.empty_like(sign)
        _launch("nesie_vote_loss_backward", sign, sign.numel(), g, scale, sign, d)
        return d

    def proposal_jitter(self, bbox, noise_c, noise_s, sigma, size_bias, zero_heading):
        """-> (centre_all (B,2K,3), size_all (B,2K,3), heading_all (B,2K), jitter_bbox (B,K,7))
        (nesie_proposal_jitter)."""
        _check(bbox, noise_c, noise_s); _f32(bbox, noise_c, noise_s)
        b, k, _ = bbox.shape
        dev = bbox.device
        f32 = lambda *s_: torch.empty(*s_, dtype=torch.float32, device=dev)  # noqa: E731
        ca, sa, ha, jb = f32(b, 2 * k, 3), f32(b, 2 * k, 3), f32(b, 2 * k), f32(b, k, 7)
        _launch("nesie_proposal_jitter", bbox, b, k, bbox, noise_c, noise_s, float(sigma),
                float(size_bias), bool(zero_heading), ca, sa, ha, jb)
        return ca, sa, ha, jb

    def side_prob_stats(self, probs, copies):
        """probs (B, 6, bins, K) -> (6, B, bins + 5, copies*K): bins, top-4, unbiased variance per
        face (nesie_side_prob_stats)."""
        _check(probs); _f32(probs)
        b, six, bins, k = probs.shape
        assert six == 6 and bins >= 5
        out = torch.empty(6, b, bins + 5, copies * k, dtype=torch.float32, device=probs.device)
        _launch("nesie_side_prob_stats", probs, b, bins, k, int(copies), probs, out)
        return out

    def flat_adamw_step(self, param, grad, exp_avg, exp_avg_sq, step, lr, betas, eps, weight_decay,
                        max_norm, grad_norm_out=None, hyper=None):
        """clip_grad_norm_(max_norm) + AdamW over flat vectors, in place (nesie_flat_adamw_step);
        ``step`` is a float32 device scalar that the call increments.  ``hyper`` (2,) device
        float32 = [lr, weight_decay]: read at execution time instead of the host values
        (nesie_flat_adamw_step_dev: a captured launch follows the schedule)."""
        _check(param, grad, exp_avg, exp_avg_sq, step); _f32(param, grad, exp_avg, exp_avg_sq, step)
        n = param.numel()
        assert grad.numel() == n == exp_avg.numel() == exp_avg_sq.numel() and step.numel() == 1
        need = _lib.load().nesie_flat_adamw_workspace_bytes()
        ws = torch.empty(need, dtype=torch.uint8, device=param.device)
        if hyper is not None:
            _check(hyper); _f32(hyper)
            assert hyper.numel() == 2 and hyper.is_contiguous()
            _launch("nesie_flat_adamw_step_dev", param, n, param, grad, exp_avg, exp_avg_sq, step,
                    hyper, float(betas[0]), float(betas[1]), float(eps), float(max_norm or 0.0),
                    grad_norm_out, ws, need)
            return
        _launch("nesie_flat_adamw_step", param, n, param, grad, exp_avg, exp_avg_sq, step,
                float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                float(max_norm or 0.0), grad_norm_out, ws, need)

    # ---- Nesie head: targets and loss terms (include/nesie_head_ops.h) -----------------------
    def head_targets(self, agg, gt_boxes, gt_labels, gt_count, gt_valid, pos_thr, neg_thr):
        """-> dict(assignment, obj_targets, obj_weights, mask_targets, bbox_targets,
        center_targets, box_weights, valid_weights) (nesie_head_targets)."""
        _check(agg, gt_boxes, gt_labels, gt_count, gt_valid); _f32(agg, gt_boxes, gt_valid)
        assert gt_labels.dtype == torch.int64 and gt_count.dtype == torch.int64
        b, k = agg.shape[:2]
        t = gt_boxes.shape[1]
        dev = agg.device
        i64 = lambda *s_: torch.empty(*s_, dtype=torch.int64, device=dev)  # noqa: E731
        f32 = lambda *s_: torch.empty(*s_, dtype=torch.float32, device=dev)  # noqa: E731
        out = dict(assignment=i64(b, k), obj_targets=i64(b, k), obj_weights=f32(b, k),
                   mask_targets=i64(b, k), bbox_targets=f32(b, k, 7), center_targets=f32(b, t, 3),
                   box_weights=f32(b, k), valid_weights=f32(b, t))
        _launch("nesie_head_targets", agg, b, k, t, agg, gt_boxes, gt_labels, gt_count, gt_valid,
                float(pos_thr), float(neg_thr), out['assignment'], out['obj_targets'],
                out['obj_weights'], out['mask_targets'], out['bbox_targets'], out['center_targets'],
                out['box_weights'], out['valid_weights'])
        return out

    def head_loss_forward(self, cls, bbox, surface, side, iou_s, iou, iou_j, tg, config, ticket,
                          quality=None, detach_sigma=False, sigma_mode=0, iou_label=None):
        """The seven loss terms + their saved gradients (nesie_head_loss_forward).  cls
        (B,2+C,K), bbox (B,K,7), surface (B,K,6), side (6,B,C,2K), iou_s (B,2K,C), iou / iou_j
        (B*K); tg = head_targets(...); config = 11 python floats; ticket = a zeroed int32 scalar
        that lives outside any graph capture (the kernel leaves it zero).  -> (loss (7,), saved dict).
        quality (B*K, 6): the unsupervised variant (nesie_head_loss_forward_unsup; iou_j unused).
        iou_label (B*K): the plain proposals' IoU-quality label where it is not ``iou`` itself
        (nesie_head_loss_forward_label; the unsupervised variant has no such term)."""
        _check(cls, bbox, surface, side, iou_s, iou, iou_j)
        _f32(cls, bbox, surface, side, iou_s, iou, iou_j)
        b, nc, k = cls.shape
        c = nc - 2
        t = tg['center_targets'].shape[1]
        assert tuple(side.shape) == (6, b, c, 2 * k) and tuple(bbox.shape) == (b, k, 7)
        assert tuple(iou_s.shape) == (b, 2 * k, c) and tuple(surface.shape) == (b, k, 6)
        assert iou.numel() == b * k == iou_j.numel() and len(config) == 11
        dev = cls.device
        f32 = lambda *s_: torch.empty(*s_, dtype=torch.float32, device=dev)  # noqa: E731
        i32 = lambda *s_: torch.empty(*s_, dtype=torch.int32, device=dev)  # noqa: E731
        sv = dict(cls=f32(b, nc, k), centre=f32(b * k, 3), surface=f32(b, k, 6), iou=f32(b * k),
                  iou_s=f32(b, 2 * k, c), side_surf=f32(b * k, 6), side_iou=f32(b * k, 6),
                  side_pred=f32(b * k, 6), sem_pick=i32(b * k))
        loss, kstar, dmin = f32(7), i32(b * t), f32(b * t)
        partial = f32((b * k + 63) // 64, 8)
        assert ticket.dtype == torch.int32 and ticket.is_cuda and ticket.numel() == 1
        cfg = (ctypes.c_float * 11)(*[float(v) for v in config])
        if quality is not None:
            _check(quality); _f32(quality)
            assert quality.numel() == b * k * 6
            head = ("nesie_head_loss_forward_unsup", cls, b, k, t, c, cls, bbox, surface, side, iou_s,
                    iou, quality, bool(detach_sigma))
        elif iou_label is not None:
            _check(iou_label); _f32(iou_label)
            assert iou_label.numel() == b * k
            head = ("nesie_head_loss_forward_label", cls, int(sigma_mode), b, k, t, c, cls, bbox,
                    surface, side, iou_s, iou, iou_label, iou_j)
        elif sigma_mode:      # the SAQE head's supervised losses: constant (1) or no (2) uncertainties
            head = ("nesie_head_loss_forward_sigma", cls, int(sigma_mode), b, k, t, c, cls, bbox,
                    surface, side, iou_s, iou, iou_j)
        else:
            head = ("nesie_head_loss_forward", cls, b, k, t, c, cls, bbox, surface, side, iou_s, iou,
                    iou_j)
        _launch(*head, tg['obj_targets'], tg['mask_targets'], tg['obj_weights'], tg['box_weights'],
                tg['bbox_targets'], tg['center_targets'], tg['valid_weights'],
                ctypes.cast(cfg, ctypes.c_void_p), loss, sv['cls'], sv['centre'], sv['surface'],
                sv['iou'], sv['iou_s'], sv['side_surf'], sv['side_iou'], sv['side_pred'],
                sv['sem_pick'], kstar, dmin, partial, ticket)
        return loss, sv

    def saqe_extra_forward(self, robj, rot, bbox, bbox_t, jsurf, side, tg, sem_pick, config, sup,
                           ticket):
        """The SAQE head's additional supervised terms (nesie_saqe_extra_loss_forward): robj
        (B,2K,2), rot (B,2K,C), bbox / bbox_t (B,K,7), jsurf (B,K,6), side (6,B,C,2K); sem_pick from
        ``head_loss_forward``; config = 7 python floats.  -> (loss (4,), saved dict)."""
        _check(robj, rot, bbox, bbox_t, jsurf, side, sem_pick); _f32(robj, rot, bbox, bbox_t, jsurf, side)
        b, k2, c = rot.shape
        k = k2 // 2
        assert tuple(robj.shape) == (b, k2, 2) and tuple(side.shape) == (6, b, c, k2) and len(config) == 7
        assert bbox.numel() == b * k * 7 == bbox_t.numel() and jsurf.numel() == b * k * 6
        dev = rot.device
        f32 = lambda *s_: torch.empty(*s_, dtype=torch.float32, device=dev)  # noqa: E731
        sv = dict(robj=f32(b, k2, 2), angle=f32(b * k), rot=torch.zeros(b, k2, c, dtype=torch.float32, device=dev),
                  sidej=f32(b * k, 6))
        loss, partial = f32(4), f32((b * k + 63) // 64, 4)
        wmax = tg['box_weights'].max().reshape(1)
        cfg = (ctypes.c_float * 7)(*[float(v) for v in config])
        _launch("nesie_saqe_extra_loss_forward", rot, b, k, c, bool(sup), robj, rot, bbox, bbox_t,
                jsurf, side, tg['obj_targets'], tg['mask_targets'], tg['obj_weights'],
                tg['box_weights'], wmax, sem_pick, ctypes.cast(cfg, ctypes.c_void_p), loss,
                sv['robj'], sv['angle'], sv['rot'], sv['sidej'], partial, ticket)
        return loss, sv

    def saqe_extra_backward(self, g, label, sv, k):
        """g (4,) -> dict(robj, angle (B*K), rot, side (6,B,C,2K))."""
        _check(g, label); _f32(g)
        b, k2, c = sv['rot'].shape
        dev = g.device
        out = dict(robj=torch.empty_like(sv['robj']), angle=torch.empty_like(sv['angle']),
                   rot=torch.empty_like(sv['rot']),
                   side=torch.zeros(6, b, c, k2, dtype=torch.float32, device=dev))
        _launch("nesie_saqe_extra_loss_backward", g, b, k, c, g, label, sv['robj'], sv['angle'],
                sv['rot'], sv['sidej'], out['robj'], out['angle'], out['rot'], out['side'])
        return out

    def head_loss_backward(self, g, label, sv, k):
        """g (7,) incoming gradients (device) -> dict(cls, bbox, surface, iou, iou_s, side) in the
        producers' layouts (nesie_head_loss_backward)."""
        _check(g, label); _f32(g)
        b, nc, _ = sv['cls'].shape
        c = nc - 2
        dev = g.device
        out = dict(cls=torch.empty_like(sv['cls']),
                   bbox=torch.empty(b, k, 7, dtype=torch.float32, device=dev),
                   surface=torch.empty_like(sv['surface']), iou=torch.empty_like(sv['iou']),
                   iou_s=torch.empty_like(sv['iou_s']),
                   side=torch.zeros(6, b, c, 2 * k, dtype=torch.float32, device=dev))
        _launch("nesie_head_loss_backward", g, b, k, c, g, label, sv['sem_pick'], sv['cls'],
                sv['centre'], sv['surface'], sv['iou'], sv['iou_s'], sv['side_surf'],
                sv['side_iou'], sv['side_pred'], out['cls'], out['bbox'], out['surface'],
                out['iou'], out['iou_s'], out['side'])
        return out

    def pw_stats_finalize(self, stat_part, gamma, beta, running_mean, running_var, momentum, eps,
                          coef, chan_bias=None):
        """(ng, slots, Cout, 4) shifted partials -> coef (ng*Cout, 4) = (scale, bias, mean,
        invstd); running statistics (ng*Cout) updated in place (or None).  chan_bias (ng*Cout):
        bias of the convolution in front of the norm, added to the running mean only."""
        _check(stat_part, coef); _f32(stat_part, coef)
        ng, nslots, cout, _ = stat_part.shape
        assert tuple(coef.shape) == (ng * cout, 4)
        assert chan_bias is None or (chan_bias.numel() == ng * cout and chan_bias.is_contiguous())
        _launch("nesie_pw_stats_finalize", coef, ng * cout, cout, nslots, stat_part, gamma, beta,
                running_mean, running_var, float(momentum), float(eps), coef, chan_bias)

    def pw_pool_finish(self, ng, p, group, pool_group, pool_out, coef, relu, pooled, argmax, zstar=None):
        """partial extrema (NB, C, P / pool_group) -> pooled (NB, C, P / group) float,
        argmax uint8 (position inside the group); zstar (optional, like pooled): the raw extremum."""
        pmax, pmin, amax, amin = pool_out
        _check(pmax, amax, pooled, argmax); _f32(pmax, pooled)
        nb, c = pooled.shape[:2]
        assert pooled.numel() == nb * c * (p // group) and argmax.dtype == torch.uint8
        if zstar is not None:
            _check(zstar); _f32(zstar)
            assert zstar.numel() == pooled.numel()
        _launch("nesie_pw_pool_finish", pooled, nb, ng, c, p, group, pool_group, pmax, pmin, amax,
                amin, coef, bool(relu), pooled, argmax, zstar)

    # ---- pooled tail without the dense pre-pool tensor (csrc/pool_tail.hip) ---------------------
    def pool_tail_supported(self, k, c, p, ns):
        return bool(_lib.load().nesie_pool_tail_supported(int(k), int(c), int(p), int(ns)))

    def pool_tail_backward(self, g, pooled, zstar, argmax, coef, gamma, w, z_prev, coef_prev, ns,
                           dgamma, dbeta, dw=None):
        """Backward of conv (k -> c) + BatchNorm + ReLU + max over groups of ``ns`` positions from
        the pooled gradient g (NB, C, M), what the forward kept (pooled, zstar, argmax (NB, C, M),
        coef (C, 4)) and the layer's operand in raw form (z_prev (NB, K, P) with its folded
        coefficients coef_prev (K, 4)).  Writes dgamma, dbeta (C,) and dw (C, K) (None: skipped);
        returns (da (NB, K, P), partials of the previous norm's backward (K, slots, 2))."""
        _check(g, pooled, zstar, argmax, coef, gamma, w, z_prev, coef_prev, dgamma, dbeta)
        _f32(g, pooled, zstar, coef, gamma, w, z_prev, coef_prev, dgamma, dbeta)
        nb, c, m = g.shape
        k, p = z_prev.shape[1], z_prev.shape[2]
        assert tuple(z_prev.shape) == (nb, k, p) and p == m * ns and tuple(w.shape) == (c, k)
        assert argmax.dtype == torch.uint8 and tuple(coef.shape) == (c, 4) and tuple(coef_prev.shape) == (k, 4)
        assert z_prev.stride(2) == 1 and z_prev.stride(1) == p
        dev = g.device
        f = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        sizes = (ctypes.c_int * 2)()
        _lib.call("nesie_pool_tail_sizes", nb, k, c, p, ctypes.addressof(sizes))   # host only: no stream
        nslots, nparts = int(sizes[0]), int(sizes[1])
        ab, ent, wcat, c0 = f(c, 4), f(nb, m, c, 2), f(k, c + k), f(k)
        da, part = f(nb, k, p), f(k, nslots, 2)
        zbs = z_prev.stride(0) if nb > 1 else k * p
        _launch("nesie_pool_tail_prepare", g, nb, c, m, ns, k, g, pooled, zstar, argmax, coef,
                gamma, w, dgamma, dbeta, ab, ent, wcat, c0)
        _launch("nesie_pool_tail_dgrad", g, nb, k, c, p, ns, z_prev, zbs, coef_prev, wcat, c0, ent,
                da, k * p, part)
        if dw is not None:
            _check(dw); _f32(dw)
            assert dw.numel() == c * k
            part_m, part_s, part_w = f(nparts, k, k), f(nparts, k), f(nparts, c, k)
            ms = torch.empty(k * k + k, dtype=torch.float64, device=dev)
            _launch("nesie_pool_tail_wgrad", g, nb, k, c, p, ns, z_prev, zbs, coef_prev, ent, ab, w,
                    part_m, part_s, part_w, ms, dw)
        return da, part

    # ---- a convolution pooled directly (MiniPointNet tail): backward from the entries -------------
    def pool_tail_pack(self, g, argmax, pooled=None):
        """g, argmax (uint8) (NB, C, M) -> ent (NB, M, C, 2) = (g -- masked by pooled > 0 when given
        --, arg-max position as int bits) (nesie_pool_tail_pack)."""
        _check(g, argmax); _f32(g)
        nb, c, m = g.shape
        assert argmax.dtype == torch.uint8 and tuple(argmax.shape) == (nb, c, m)
        if pooled is not None:
            _check(pooled); _f32(pooled)
            assert tuple(pooled.shape) == (nb, c, m)
        ent = torch.empty(nb, m, c, 2, dtype=torch.float32, device=g.device)
        _launch("nesie_pool_tail_pack", g, nb, c, m, g, pooled, argmax, ent)
        return ent

    def pw_dgrad_bn_reduce_sparse(self, ent, ns, w, z, z_coef, da, ng=1):
        """``pw_dgrad_bn_reduce`` whose dy (NB, 128, P) is given as the entries of a max over groups of
        ``ns`` positions, ent (NB, P / ns, 128, 2) (nesie_pw_dgrad_bn_reduce_sparse): bit for bit the
        dense launch's da and partials."""
        _check(ent, z_coef); _f32(ent, w, z, da, z_coef)
        nb, cout, p = z.shape
        k = 128
        assert tuple(ent.shape) == (nb, p // ns, k, 2) and p % ns == 0
        assert w.dim() == 3 and w.shape[0] == ng and w.shape[1] == cout and w.shape[2] == k and nb % ng == 0
        for t in (z, da):
            assert t.is_cuda and t.stride(2) == 1 and t.stride(1) == p
        assert tuple(da.shape) == (nb, cout, p) and tuple(z_coef.shape) == (ng * cout, 4)
        part = torch.empty(ng * cout, self.pw_stat_slots(nb, ng, k, cout, p), 2,
                           dtype=torch.float32, device=z.device)
        bs = lambda t, rows: t.stride(0) if nb > 1 else rows * p  # noqa: E731
        _launch("nesie_pw_dgrad_bn_reduce_sparse", z, nb, ng, k, cout, p, int(ns), ent, w,
                w.stride(0) if ng > 1 else 0, w.stride(1), w.stride(2), da, bs(da, cout), z,
                bs(z, cout), z_coef, part)
        return part

    def pw_wgrad_sparse_supported(self, co, ci, p, ns):
        return bool(_lib.load().nesie_pw_wgrad_sparse_supported(int(co), int(ci), int(p), int(ns)))

    def pw_wgrad_sparse(self, ent, ns, x, dw, ng=1, x_coef=None, final=False):
        """``pw_wgrad`` whose dy (NB, 128, P) is given as the entries of a max over groups of ``ns``
        positions, ent (NB, P / ns, 128, 2) (nesie_pw_wgrad_sparse): dw (ng, 128, ci) bit for bit the
        dense launch's; x (NB, ci, P) raw, x_coef (ng*ci, 4) its folded BatchNorm (ReLU applied)."""
        _check(ent, x_coef); _f32(ent, x, x_coef, dw)
        nb, ci, p = x.shape
        co = ent.shape[2]
        assert tuple(ent.shape) == (nb, p // ns, co, 2) and p % ns == 0 and nb % ng == 0
        assert x.is_cuda and x.stride(2) == 1 and x.stride(1) == p
        assert dw.is_contiguous() and dw.numel() == ng * co * ci and tuple(x_coef.shape) == (ng * ci, 4)
        ws, need, defer = self._wgrad_scratch(nb, ng, co, ci, p, dw, final)
        _launch("nesie_pw_wgrad_sparse", x, nb, ng, co, ci, p, int(ns), ent, x,
                x.stride(0) if nb > 1 else ci * p, x_coef, dw, ws, need, defer)

    def mlp_stat_finalize(self, part, count, gamma, beta, running_mean, running_var, momentum, eps,
                          coef, channel_major=False):
        """(parts, C, 2) -- or, channel_major, (C, parts, 2) -- unshifted (sum, sum of squares)
        partials -> coef (C, 4); running statistics updated in place."""
        _check(part, coef); _f32(part, coef)
        if channel_major:
            c, nparts, _ = part.shape
        else:
            nparts, c, _ = part.shape
        _launch("nesie_mlp_stat_finalize", coef, c, nparts, float(count), part, gamma, beta,
                running_mean, running_var, float(momentum), float(eps), coef, bool(channel_major))

    def bn_relu_backward(self, dy, x, y, gamma, beta, save_mean, save_invstd, fwd_coef, relu,
                         dx, dgamma, dbeta, row_bias=None, d_row_bias=None, group=None):
        """y None with relu: x is the raw conv output of a fused forward (mask re-derived from
        fwd_coef).  d_row_bias without row_bias (+ ``group``): per-group sums of dx.
        save_mean / save_invstd None: columns 2 / 3 of fwd_coef."""
        _check(dy, x, dx, fwd_coef); _f32(dy, x, dx)
        assert (save_mean is None) == (save_invstd is None)
        if save_mean is not None:
            _check(save_mean, save_invstd)
        b, c = x.shape[:2]
        p = x.numel() // (b * c) if b * c else 0
        if row_bias is None and d_row_bias is not None:
            _check(d_row_bias); _f32(d_row_bias)
            assert group and d_row_bias.numel() == b * c * (p // group)
        else:
            group = _row_bias_group(x, row_bias)
        if row_bias is not None and row_bias.dim() != 1:
            _check(d_row_bias); _f32(d_row_bias)
            assert d_row_bias.shape == row_bias.shape
        elif row_bias is not None:
            assert d_row_bias is None  # per-channel bias before a batch norm: gradient is zero
        need = _lib.load().nesie_bn_workspace_bytes(b, c, p)
        ws = _workspace(need, x.device)
        _launch("nesie_bn_relu_backward", x, b, c, p, dy, x, y, gamma, beta, save_mean, save_invstd,
                fwd_coef, bool(relu), dx, dgamma, dbeta, row_bias, group, d_row_bias, ws, need)

    # ---- synchronised norm: the caller all-reduces ``moments`` / ``sums`` between each pair ----
    @staticmethod
    def _syncbn_dims(x, *same):
        _check(x, *same); _f32(x, *same)
        assert x.dim() >= 2 and all(t.shape == x.shape for t in same)
        b, c = x.shape[:2]
        return b, c, (x.numel() // (b * c) if b * c else 0)

    @staticmethod
    def _f64(t, shape):
        _check(t)
        if t.dtype != torch.float64 or tuple(t.shape) != shape:
            raise TypeError(f"expected float64 {shape}, got {t.dtype} {tuple(t.shape)}")

    def syncbn_local_moments(self, x, moments):
        """moments (C, 3) float64 <- (n_local, sum x, sum x^2) of x (B, C, *) per channel."""
        b, c, p = self._syncbn_dims(x)
        self._f64(moments, (c, 3))
        need = _lib.load().nesie_syncbn_workspace_bytes(b, c, p)
        ws = _workspace(need, x.device)
        _launch("nesie_syncbn_local_moments", x, b, c, p, x, moments, ws, need)

    def syncbn_forward_apply(self, x, moments, gamma, beta, running_mean, running_var, momentum,
                             eps, relu, y, fwd_coef):
        """y, fwd_coef (C, 4) and the running statistics from the all-reduced ``moments``."""
        b, c, p = self._syncbn_dims(x, y)
        self._f64(moments, (c, 3))
        _check(fwd_coef); _f32(fwd_coef)
        assert tuple(fwd_coef.shape) == (c, 4)
        for v in (gamma, beta, running_mean, running_var):
            if v is not None:
                _check(v); _f32(v)
                assert v.numel() == c
        _launch("nesie_syncbn_forward_apply", x, b, c, p, x, moments, gamma, beta, running_mean,
                running_var, float(momentum), float(eps), bool(relu), y, fwd_coef)

    def syncbn_backward_local(self, dy, x, fwd_coef, moments, eps, relu, sums, dgamma, dbeta):
        """sums (C, 2) float64 <- (sum g, sum g * xhat) over this rank; dgamma, dbeta: the same
        local sums in fp32.  ``moments``: the reduced ones of the forward; ``eps``: its eps."""
        b, c, p = self._syncbn_dims(x, dy)
        self._f64(sums, (c, 2)); self._f64(moments, (c, 3))
        _check(fwd_coef, dgamma, dbeta); _f32(fwd_coef, dgamma, dbeta)
        assert tuple(fwd_coef.shape) == (c, 4) and dgamma.numel() == c and dbeta.numel() == c
        need = _lib.load().nesie_syncbn_workspace_bytes(b, c, p)
        ws = _workspace(need, x.device)
        _launch("nesie_syncbn_backward_local", x, b, c, p, dy, x, fwd_coef, moments, float(eps),
                bool(relu), sums, dgamma, dbeta, ws, need)

    def syncbn_backward_apply(self, dy, x, fwd_coef, gamma, sums, moments, eps, relu, dx):
        """dx from the all-reduced ``sums`` and the reduced ``moments``."""
        b, c, p = self._syncbn_dims(x, dy, dx)
        self._f64(sums, (c, 2)); self._f64(moments, (c, 3))
        _check(fwd_coef); _f32(fwd_coef)
        assert tuple(fwd_coef.shape) == (c, 4) and (gamma is None or gamma.numel() == c)
        _launch("nesie_syncbn_backward_apply", x, b, c, p, dy, x, fwd_coef, gamma, sums, moments,
                float(eps), bool(relu), dx)

    def assign_score_withk_forward(self, b, n0, n1, m, k, o, points, centers, scores, knn_idx,
                                   output):
        """output (B, O, N1, K) <- sum_m scores * (points[knn_idx] - centers[knn_idx[..., 0]]),
        WRITTEN in full (nesie_assign_score_withk_forward; the size order is the reference
        wrapper's B, N0, N1, M, K, O)."""
        _check(points, centers, scores, knn_idx, output); _f32(points, centers, scores, output)
        if knn_idx.dtype != torch.int64:
            raise TypeError(f"expected int64, got {knn_idx.dtype}")
        assert points.numel() == b * n0 * m * o and centers.numel() == b * n0 * m * o
        assert scores.numel() == b * n1 * k * m and knn_idx.numel() == b * n1 * k
        assert output.numel() == b * o * n1 * k
        _launch("nesie_assign_score_withk_forward", output, b, n0, n1, k, m, o, points, centers,
                scores, knn_idx, output)

    def assign_score_withk_backward(self, b, n0, n1, m, k, o, grad_out, points, centers, scores,
                                    knn_idx, grad_points, grad_centers, grad_scores):
        """grad_points / grad_centers (B, N0, M, O) and grad_scores (B, N1, K, M), each WRITTEN in
        full in a fixed order, or None = skipped (nesie_assign_score_withk_backward)."""
        _check(grad_out, points, centers, scores, knn_idx); _f32(grad_out, points, centers, scores)
        if knn_idx.dtype != torch.int64:
            raise TypeError(f"expected int64, got {knn_idx.dtype}")
        assert points.numel() == b * n0 * m * o and centers.numel() == b * n0 * m * o
        assert scores.numel() == b * n1 * k * m and knn_idx.numel() == b * n1 * k
        assert grad_out.numel() == b * o * n1 * k
        for g, like in ((grad_points, points), (grad_centers, centers), (grad_scores, scores)):
            if g is not None:
                _check(g); _f32(g)
                assert g.numel() == like.numel()
        need = _lib.load().nesie_assign_score_withk_backward_workspace_bytes(b, n0, n1, k, m, o)
        ws = _workspace(need, grad_out.device)
        _launch("nesie_assign_score_withk_backward", grad_out, b, n0, n1, k, m, o, grad_out, points,
                centers, scores, knn_idx, grad_points, grad_centers, grad_scores, ws, need)

    @staticmethod
    def _focal_operands(input, target, weight, sample_weight):
        """Checks of the operands the three focal-loss entries share -> (n, c, sample-weight mode:
        0 none, 1 one weight per row (N,), 2 one per element (N, C) or any shape of N * C)."""
        _check(input, target); _f32(input)
        if target.dtype != torch.int64:
            raise TypeError(f"expected int64, got {target.dtype}")
        assert input.dim() == 2 and target.numel() == input.shape[0]
        n, c = input.shape
        if weight is not None:
            _check(weight); _f32(weight)
            assert weight.numel() == c
        mode = 0
        if sample_weight is not None:
            _check(sample_weight); _f32(sample_weight)
            assert sample_weight.numel() in (n, n * c)
            mode = 1 if sample_weight.numel() == n else 2
        return n, c, mode

    def sigmoid_focal_loss_forward(self, input, target, weight, output, gamma, alpha,
                                   sample_weight=None, scale=1.0):
        """output (N, C) <- focal term * weight[target] * sample_weight * scale, WRITTEN in full
        (nesie_sigmoid_focal_loss_forward; the leading six arguments are mmcv's)."""
        n, c, mode = self._focal_operands(input, target, weight, sample_weight)
        _check(output); _f32(output)
        assert output.numel() == n * c
        _launch("nesie_sigmoid_focal_loss_forward", input, n, c, input, target, weight,
                sample_weight, mode, float(gamma), float(alpha), float(scale), output)

    def sigmoid_focal_loss_forward_sum(self, input, target, weight, output, gamma, alpha,
                                       sample_weight=None, scale=1.0, scale_dev=None):
        """output (one element) <- sum of the weighted focal terms * scale * scale_dev[0], in a
        fixed order; the (N, C) loss is never stored (nesie_sigmoid_focal_loss_forward_sum)."""
        n, c, mode = self._focal_operands(input, target, weight, sample_weight)
        _check(output); _f32(output)
        assert output.numel() == 1
        if scale_dev is not None:
            _check(scale_dev); _f32(scale_dev)
            assert scale_dev.numel() == 1
        need = _lib.load().nesie_sigmoid_focal_loss_workspace_bytes(n, c)
        ws = _workspace(need, input.device) if need else None    # a single chunk needs no scratch
        _launch("nesie_sigmoid_focal_loss_forward_sum", input, n, c, input, target, weight,
                sample_weight, mode, float(gamma), float(alpha), float(scale), scale_dev, output,
                ws, need)

    def sigmoid_focal_loss_backward(self, input, target, weight, grad_input, gamma, alpha,
                                    sample_weight=None, grad_output=None, grad_scalar=None,
                                    scale=1.0, scale_dev=None):
        """grad_input (N, C) <- d term/d input * weights * upstream, WRITTEN in full in one launch;
        upstream is grad_output (N, C) or the one-element grad_scalar, read on the device, times
        scale * scale_dev[0] (nesie_sigmoid_focal_loss_backward)."""
        n, c, mode = self._focal_operands(input, target, weight, sample_weight)
        _check(grad_input); _f32(grad_input)
        assert grad_input.numel() == n * c
        assert (grad_output is None) != (grad_scalar is None)
        for t, count in ((grad_output, n * c), (grad_scalar, 1), (scale_dev, 1)):
            if t is not None:
                _check(t); _f32(t)
                assert t.numel() == count
        _launch("nesie_sigmoid_focal_loss_backward", input, n, c, input, target, weight,
                sample_weight, mode, float(gamma), float(alpha), grad_output, grad_scalar,
                float(scale), scale_dev, grad_input)

    @staticmethod
    def lovasz_softmax_workspace_bytes(images, classes, points):
        """Scratch bytes of ``lovasz_softmax`` (nesie_lovasz_softmax_workspace_bytes); 0 for an
        empty problem and for one the kernels refuse."""
        return _lib.load().nesie_lovasz_softmax_workspace_bytes(images, classes, points)

    def lovasz_softmax(self, probas, labels, loss, grad, per_image=False, ignore=None,
                       class_mode=1, class_mask=None, workspace=None):
        """probas (B, C, S) float32 of ANY non-overlapping strides, labels (B, S) int64 -> loss (one
        element) and grad (B, C, S, the strides of probas), both WRITTEN in full
        (nesie_lovasz_softmax).  class_mode 0 all / 1 present / 2 ``class_mask`` (C int32 counts)."""
        for t in (probas, grad):
            if not t.is_cuda:
                raise _no_cpu_path(t.device)
        _check(labels, loss); _f32(probas, loss, grad)
        if labels.dtype != torch.int64:
            raise TypeError(f"expected int64, got {labels.dtype}")
        assert probas.dim() == 3 and tuple(labels.shape) == (probas.shape[0], probas.shape[2])
        assert grad.shape == probas.shape and grad.stride() == probas.stride()
        assert loss.numel() == 1 and class_mode in (0, 1, 2)
        b, c, s = probas.shape
        if class_mode == 2:
            _check(class_mask); _i32(class_mask)
            assert class_mask.numel() == c
        else:
            class_mask = None
        need = self.lovasz_softmax_workspace_bytes(b, c, s)
        workspace = self._voxel_workspace(workspace, need, probas.device)
        sb, sc, ss = probas.stride()
        _launch("nesie_lovasz_softmax", probas, b, c, s, probas, sb, sc, ss, labels,
                ignore is not None, 0 if ignore is None else int(ignore), bool(per_image),
                int(class_mode), class_mask, loss, grad, workspace, need)


def _row_bias_group(x, row_bias):
    if row_bias is None:
        return 1
    _check(row_bias); _f32(row_bias)
    if row_bias.dim() == 1:  # one value per channel (a conv bias folded into the norm): group 0
        assert row_bias.shape[0] == x.shape[1], (tuple(x.shape), tuple(row_bias.shape))
        return 0
    assert x.dim() == 4 and tuple(row_bias.shape) == tuple(x.shape[:3]), \
        (tuple(x.shape), tuple(row_bias.shape))
    return int(x.shape[3])


_hip = None


def backend_for(tensor):
    """The back end that serves ``tensor``: injected one, else HIP (or raise)."""
    global _hip
    if _injected is not None:
        return _injected
    if not tensor.is_cuda:
        raise RuntimeError(
            f"nesie_amd op called on a {tensor.device} tensor: the product path is "
            "HIP-only (libnesie_hip.so); there is no CPU fallback")
    if _hip is None:
        _lib.load()
        _hip = HipKernels()
    return _hip


def injected_backend():
    return _injected


@contextlib.contextmanager
def spatial_index_scope():
    """One sample-then-group pass over ONE coordinate tensor (a set-abstraction forward): the
    spatial index the FPS kernel leaves behind may serve the ball queries inside this block and
    nothing after it."""
    HipKernels._index_scope_depth += 1
    try:
        yield
    finally:
        HipKernels._index_scope_depth -= 1
        if HipKernels._index_scope_depth == 0:
            HipKernels._spatial_index.clear()


@contextlib.contextmanager
def use_backend(backend):
    """Test/bench hook: run the enclosed code with ``backend`` serving every op."""
    global _injected
    prev = _injected
    _injected = backend
    try:
        yield backend
    finally:
        _injected = prev
