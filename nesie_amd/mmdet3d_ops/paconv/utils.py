"""The torch-only helpers of ``mmdet3d/ops/paconv/utils.py:4-86``; any device, any float dtype."""
import torch


def calc_euclidian_dist(xyz1, xyz2):
    """xyz1, xyz2 (N, 3) -> (N,) distance of every pair of rows."""
    assert xyz1.shape[0] == xyz2.shape[0], 'number of points are not the same'
    assert xyz1.shape[1] == xyz2.shape[1] == 3, 'points coordinates dimension is not 3'
    return torch.norm(xyz1 - xyz2, dim=-1)


def assign_score(scores, point_features):
    """scores (B, npoint, K, M), point_features (B, npoint, K, M, out_dim) ->
    (B, npoint, K, out_dim): every pair's M bank outputs blended by its scores.  This is what
    the non-kernel ``PAConv`` runs; it needs the (B, npoint, K, M, out_dim) operand in memory,
    which ``assign_score_withk`` never forms."""
    B, npoint, K, M = scores.size()
    blended = torch.matmul(scores.view(B, npoint, K, 1, M), point_features)
    return blended.view(B, npoint, K, -1)


def assign_kernel_withoutk(features, kernels, M):
    """features (B, in_dim, N), kernels (2 * in_dim, M * out_dim) -> (point_features,
    center_features), both (B, N, M, out_dim): the bank applied to every point once, split so
    that ``point_features[neighbour] - center_features[centre]`` is the bank applied to
    ``cat(feature difference, neighbour feature)``.

    The reference's quirk is kept (utils.py:72-82): with an ODD ``in_dim`` (bare xyz as the
    features) the centre half also receives the first three channels through rows
    ``in_dim .. in_dim + 3`` of the bank."""
    B, in_dim, N = features.size()
    rows = features.permute(0, 2, 1)                       # (B, N, in_dim)
    diff_half = torch.matmul(rows, kernels[:in_dim]).view(B, N, M, -1)
    self_half = torch.matmul(rows, kernels[in_dim:]).view(B, N, M, -1)
    if in_dim % 2 != 0:
        coord_half = torch.matmul(rows[:, :, :3], kernels[in_dim:in_dim + 3]).view(B, N, M, -1)
    else:
        coord_half = torch.zeros_like(self_half)
    return diff_half + self_half, diff_half + coord_half
