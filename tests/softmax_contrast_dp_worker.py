"""One rank of the global-batch check of `SoftmaxContrastiveLoss` (launched by tests/test_softmax_contrast_gpu.py, never
collected by pytest).

Every rank builds the same seeded global batch (B pairs, group ids in [0, 4)), takes its contiguous shard and runs the
module with `group=` the gloo world group (the ranks share the test box's one GPU): loss, the shard's gradients and
the temperature gradient of `3·loss` go to `$CMHAR_SMC_OUT/rank{r}.pt`.  Rank 0 also runs the whole batch in one
process (`group=False`) and writes `full.pt`."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'crossmodal-imu-video-ood-har_amd'))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def run(lf, a, b, ids):
    a, b = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    lf.zero_grad(set_to_none=True)
    loss = lf(a, b, labels=ids)
    (loss * 3).backward()
    return {'loss': loss.detach().cpu(), 'da': a.grad.cpu(), 'db': b.grad.cpu(), 'gt': lf.temperature.grad.cpu()}


def main():
    from cmhar.losses import SoftmaxContrastiveLoss
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    out = os.environ['CMHAR_SMC_OUT']
    mode = os.environ['CMHAR_SMC_MODE']
    dist.init_process_group('gloo', rank=rank, world_size=world)
    B, D = 65 * world, 100
    g = torch.Generator().manual_seed(5)
    a = F.normalize(torch.randn(B, D, generator=g), dim=1).cuda()
    b = F.normalize(a.cpu() + 0.3 * torch.randn(B, D, generator=g), dim=1).cuda()
    ids = torch.randint(0, 4, (B,), generator=g)
    sl = slice(rank * B // world, (rank + 1) * B // world)
    lf = SoftmaxContrastiveLoss(same_group=mode, group=dist.group.WORLD).cuda()
    torch.save(run(lf, a[sl], b[sl], ids[sl]), os.path.join(out, f'rank{rank}.pt'))
    if rank == 0:
        torch.save(run(SoftmaxContrastiveLoss(same_group=mode, group=False).cuda(), a, b, ids),
                   os.path.join(out, 'full.pt'))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
