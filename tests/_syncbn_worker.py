"""One rank of the synchronised-norm GPU tests (tests/test_syncbn_gpu.py starts it with
subprocess; RANK / WORLD_SIZE / MASTER_* and the back-end switches come from the environment).

    python tests/_syncbn_worker.py module OUT_DIR    one rank, NESIE_FORCE_PG=1, RCCL
    python tests/_syncbn_worker.py shards OUT_DIR    two ranks on one GPU, NESIE_DIST_BACKEND=gloo

It writes OUT_DIR/rank<r>.pt for the parent to compare and ends at its first error with a non-zero
status."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

MODULE_SHAPE = (4, 32, 30, 16)
LAYER_SHAPES = [(3, 37, 250), (1, 37, 250)]
LEVEL = dict(num_point=64, radius=0.4, num_sample=16, mlp_channels=[3, 32, 32, 64])


def level_inputs():
    """Two 1024-point scenes: xyz (2, 1024, 3), features (2, 3, 1024) = the coordinates themselves,
    and the weights (2, 64, 64) of the scalar the gradient is taken of."""
    from tests import _small
    pts, _, _ = _small.small_batch(seed=7, batch=2, n=1024)
    xyz = pts[:, :, :3].contiguous()
    w = torch.randn(2, 64, 64, generator=torch.Generator().manual_seed(5))
    return xyz, xyz.transpose(1, 2).contiguous(), w


def run_layer(layer, x, go, dev):
    x = x.to(dev).requires_grad_(True)
    y = layer(x)
    y.backward(go.to(dev))
    return dict(y=y.detach().cpu(), dx=x.grad.cpu(), dgamma=layer.weight.grad.cpu(),
                dbeta=layer.bias.grad.cpu(), running_mean=layer.running_mean.cpu(),
                running_var=layer.running_var.cpu(), tracked=int(layer.num_batches_tracked))


def load(layer, gamma, beta):
    with torch.no_grad():
        layer.weight.copy_(gamma)
        layer.bias.copy_(beta)
    return layer


def main(mode, out_dir):
    from nesie_amd import dp
    from nesie_amd.mmdet3d_ops import NaiveSyncBatchNorm1d, NaiveSyncBatchNorm2d, PointSAModule
    from tests import _syncbn_ref as R
    rank, world, _ = dp.init_distributed()
    assert dist.is_initialized(), 'no process group: NESIE_FORCE_PG / WORLD_SIZE not set'
    dev = torch.device('cuda:0')
    out = dict(backend=dist.get_backend(), world=world)
    if mode == 'module':
        assert world == 1 and dp.force_process_group()
        (x,), (go,), gamma, beta = R.make_inputs([MODULE_SHAPE], seed=21)
        layer = load(NaiveSyncBatchNorm2d(MODULE_SHAPE[1], relu=True), gamma, beta).to(dev)
        out['module'] = run_layer(layer, x, go, dev)
        # the collective is not captured: the sync path refuses a capturing stream, naming the layer
        xg = x.to(dev)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph, capture_error_mode='thread_local'):
                layer(xg)
            out['capture'] = 'accepted'
        except RuntimeError as e:
            out['capture'] = str(e)
        torch.cuda.synchronize()
    elif mode == 'shards':
        assert world == 2
        xs, gos, gamma, beta = R.make_inputs(LAYER_SHAPES, seed=22)          # the same on both ranks
        layer = load(NaiveSyncBatchNorm1d(LAYER_SHAPES[0][1], relu=True), gamma, beta).to(dev)
        out['layer'] = run_layer(layer, xs[rank], gos[rank], dev)
        # one set-abstraction level, built synchronised, one scene per rank
        xyz, feats, w = level_inputs()
        torch.manual_seed(0)                                                 # the same weights on both ranks
        sa = PointSAModule(norm_cfg=dict(type='naiveSyncBN2d'), **LEVEL)
        out['state'] = {k: v.clone() for k, v in sa.state_dict().items()}
        sa = sa.to(dev)
        f = feats[rank:rank + 1].to(dev).requires_grad_(True)
        _, pooled, idx = sa(xyz[rank:rank + 1].to(dev), f)
        (pooled * w[rank:rank + 1].to(dev)).sum().backward()
        out['level'] = dict(pooled=pooled.detach().cpu(), dfeat=f.grad.cpu(), idx=idx.cpu())
    else:
        raise SystemExit(f'unknown mode {mode}')
    torch.cuda.synchronize()
    torch.save(out, os.path.join(out_dir, f'rank{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main(sys.argv[1], sys.argv[2])
