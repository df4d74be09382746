"""Writes tests/golden/voxel.npz: inputs and outputs of the reference's CPU voxelizers
``hard_voxelize_cpu`` and ``dynamic_voxelize_cpu`` (mmdet3d/ops/voxel/src/voxelization_cpu.cpp).

    python tests/golden/make_voxel_golden.py /path/to/reference

The reference's source is compiled from ITS path into a scratch directory at generation time,
behind the small binding below (ours); nothing of the reference is copied into this repository,
and nothing is built when the tests run.  tests/test_voxel_cpu.py holds the numpy referee
(tests/_voxel_ref.py) to these arrays bit for bit.
"""
import os
import sys
import tempfile

import numpy as np
import torch

BINDING = r'''
#include <torch/extension.h>
#include <vector>
#include "%(source)s"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("hard_voxelize",
        [](const at::Tensor &points, at::Tensor &voxels, at::Tensor &coors, at::Tensor &num,
           std::vector<float> voxel_size, std::vector<float> coors_range, int max_points,
           int max_voxels) {
          return voxelization::hard_voxelize_cpu(points, voxels, coors, num, voxel_size,
                                                 coors_range, max_points, max_voxels, 3);
        });
  m.def("dynamic_voxelize",
        [](const at::Tensor &points, at::Tensor &coors, std::vector<float> voxel_size,
           std::vector<float> coors_range) {
          voxelization::dynamic_voxelize_cpu(points, coors, voxel_size, coors_range, 3);
        });
}
'''

ROOM = ([0.25, 0.25, 0.25], [-4.0, -4.0, 0.0, 4.0, 4.0, 3.0])          # 32 x 32 x 12
LIDAR = ([0.05, 0.05, 0.1], [0.0, -40.0, -3.0, 70.4, 40.0, 1.0])        # 1408 x 1600 x 40
TINY = ([1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 2.0, 2.0, 1.0])               # 2 x 2 x 1


def cloud(rng, n, c, coors_range, margin=0.0):
    lo, hi = np.asarray(coors_range[:3]), np.asarray(coors_range[3:])
    pts = rng.uniform(0, 1, (n, c)).astype(np.float32)
    pts[:, :3] = (lo - margin + pts[:, :3] * (hi - lo + 2 * margin)).astype(np.float32)
    return pts


def cases():
    """name -> (points, voxel_size, coors_range, max_points, max_voxels)"""
    rng = np.random.default_rng(20240607)
    out = {}
    out['room_cap_midstream'] = (cloud(rng, 3000, 4, ROOM[1], 0.5), *ROOM, 5, 200)
    out['room_more_voxels_than_cells'] = (cloud(rng, 3000, 5, ROOM[1], 0.5), *ROOM, 3, 20000)
    out['lidar_sparse'] = (cloud(rng, 2500, 4, LIDAR[1], 1.0), *LIDAR, 5, 1500)
    out['tiny_grid'] = (cloud(rng, 700, 3, TINY[1], 0.25), *TINY, 5, 8)
    one = cloud(rng, 400, 4, ROOM[1])
    one[:, :3] = np.float32([1.05, -2.45, 0.55]) + rng.uniform(0, 0.1, (400, 3)).astype(np.float32)
    out['one_cell_max1'] = (one, *ROOM, 1, 50)
    out['one_cell_max5'] = (one.copy(), *ROOM, 5, 50)
    outside = cloud(rng, 300, 4, ROOM[1])
    outside[:, 2] += 10.0
    out['all_out_of_range'] = (outside, *ROOM, 5, 50)
    edge = cloud(rng, 64, 4, ROOM[1])
    lo, hi = np.float32(ROOM[1][:3]), np.float32(ROOM[1][3:])
    edge[0, :3] = lo                                        # on lo: inside
    edge[1, :3] = hi                                        # on hi: outside
    edge[2, :3] = [hi[0], 0.0, 1.0]
    edge[3, :3] = [np.nextafter(hi[0], np.float32(0)), 0.0, 1.0]
    edge[4, :3] = [np.nextafter(lo[0], np.float32(-10)), 0.0, 1.0]
    edge[5, :3] = [0.0, 0.0, -0.0]                          # -0.0 - 0.0 = -0.0: cell 0
    edge[6, :3] = [np.nan, 0.0, 1.0]
    edge[7, :3] = [0.0, np.inf, 1.0]
    edge[8, :3] = [0.0, 0.0, -np.inf]
    edge[9, :3] = [3e38, 0.0, 1.0]
    edge[10, :3] = [0.0, -3e38, 1.0]
    edge[11, :3] = [0.25, 0.5, 0.75]                        # on cell planes
    out['edges_and_specials'] = (edge, *ROOM, 4, 64)
    return out


def main(reference):
    source = os.path.join(os.path.abspath(reference),
                          'mmdet3d/ops/voxel/src/voxelization_cpu.cpp')
    if not os.path.exists(source):
        raise SystemExit(f'{source} not found')
    from torch.utils.cpp_extension import load
    with tempfile.TemporaryDirectory() as scratch:
        binding = os.path.join(scratch, 'voxel_golden_binding.cpp')
        with open(binding, 'w') as f:
            f.write(BINDING % {'source': source})
        ext = load(name='voxel_golden_ref', sources=[binding], build_directory=scratch,
                   extra_cflags=['-O2', '-ffp-contract=off'], with_cuda=False, verbose=False)
        arrays = {'names': np.array(sorted(cases()))}
        for name, (points, vs, cr, max_points, max_voxels) in cases().items():
            pts = torch.from_numpy(points)
            dyn = torch.zeros((pts.shape[0], 3), dtype=torch.int32)
            ext.dynamic_voxelize(pts, dyn, vs, cr)
            voxels = torch.zeros((max_voxels, max_points, pts.shape[1]))
            coors = torch.zeros((max_voxels, 3), dtype=torch.int32)
            num = torch.zeros((max_voxels,), dtype=torch.int32)
            m = ext.hard_voxelize(pts, voxels, coors, num, vs, cr, max_points, max_voxels)
            arrays.update({
                f'{name}/points': points,
                f'{name}/voxel_size': np.float32(vs),
                f'{name}/coors_range': np.float32(cr),
                f'{name}/max_points': np.int32(max_points),
                f'{name}/max_voxels': np.int32(max_voxels),
                f'{name}/dynamic_coors': dyn.numpy(),
                f'{name}/voxels': voxels[:m].numpy(),
                f'{name}/coors': coors[:m].numpy(),
                f'{name}/num_points_per_voxel': num[:m].numpy(),
            })
            print(f'{name}: {pts.shape[0]} points -> {m} voxels')
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'voxel.npz')
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
