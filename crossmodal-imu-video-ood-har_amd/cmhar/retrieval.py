"""Similarity top-k and cross-modal retrieval recall@k on the fused kernel (`cmhar_sim_topk`, csrc/sim_topk.hip).

The reference trains its IMU↔video pair with a SigLIP / InfoNCE loss and reports the loss only; the first number
asked of such a pair is retrieval: for each IMU window, is its own video clip among the k most similar clips (and the
other way round)?  `sim_topk` is the primitive (the k largest dot products of each query row against a bank, with
indices, without ever storing the N×M scores); `recall_at_k` and `evaluate_retrieval` are built on it, and so is the
k-NN OOD detector of `cmhar.ood`.  There is no torch fallback: a shape the kernel refuses raises.
"""
from __future__ import annotations

import torch

from . import _lib as L

_DTYPES = (torch.float32, torch.bfloat16, torch.float16)
MAX_K = 64


def sim_topk(queries: torch.Tensor, bank: torch.Tensor, k: int, self_offset=None):
    """(values fp32 [N, k], indices int64 [N, k]): the k largest `queries[i] · bank[j]` per query row, descending,
    equal scores by ascending bank index.  `self_offset` (int) leaves bank row `self_offset + i` out of query i's
    candidates — leave-one-out scoring of a bank (0), or of the slice `bank[o:o+N]` (o), against the bank itself.
    Device 2-D tensors of one dtype (fp32 / bf16 / fp16) and one width d, 32 <= d <= 1024, d % 32 == 0; k <= 64."""
    if not (isinstance(queries, torch.Tensor) and isinstance(bank, torch.Tensor)):
        raise ValueError('queries and bank must be tensors')
    if queries.dim() != 2 or bank.dim() != 2 or not queries.is_cuda or queries.device != bank.device:
        raise ValueError('expected two 2-D tensors on one GPU')
    if queries.dtype != bank.dtype:
        raise ValueError(f'queries ({queries.dtype}) and bank ({bank.dtype}) must have one dtype')
    if queries.dtype not in _DTYPES:
        raise ValueError(f'unsupported dtype {queries.dtype} (fp32, bf16 or fp16)')
    N, d = queries.shape
    M = bank.shape[0]
    if bank.shape[1] != d:
        raise ValueError(f'width mismatch: queries {d}, bank {bank.shape[1]}')
    if d < 32 or d > 1024 or d % 32 != 0:
        raise ValueError(f'd = {d} is outside the supported range (32..1024, a multiple of 32)')
    k = int(k)
    so = -1 if self_offset is None else int(self_offset)
    if so < -1:
        raise ValueError('self_offset must be >= 0 (or None)')
    if N < 1:
        raise ValueError('no queries')
    if k < 1 or k > MAX_K:
        raise ValueError(f'k = {k} is outside 1..{MAX_K}')
    if k > M - (1 if so >= 0 else 0):
        raise ValueError(f'k = {k} exceeds the {M - (1 if so >= 0 else 0)} candidates per query')
    align = 16 // queries.element_size()

    def rows(t):            # unit inner stride, 16-byte aligned rows
        if t.stride(1) != 1 or t.stride(0) % align != 0 or t.stride(0) < d or t.data_ptr() % 16 != 0:
            t = t.contiguous()
        return t
    queries, bank = rows(queries), rows(bank)
    dev = queries.device
    vals = torch.empty(N, k, dtype=torch.float32, device=dev)
    idx = torch.empty(N, k, dtype=torch.int32, device=dev)
    nbytes = L.lib().cmhar_sim_topk_ws(N, M, k)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    with torch.cuda.device(dev):
        L.call('cmhar_sim_topk', L.dtype_code(queries.dtype), N, M, d, k, queries.data_ptr(), queries.stride(0),
               bank.data_ptr(), bank.stride(0), so, vals.data_ptr(), idx.data_ptr(), L.ptr(ws), L.stream(dev))
    return vals, idx.long()


def _directed_recall(q, bank, ks):
    idx = sim_topk(q, bank, max(ks))[1]
    hit = idx == torch.arange(q.shape[0], device=q.device).unsqueeze(1)     # row i's positive is bank row i
    hits = torch.stack([hit[:, :k].any(1).sum() for k in ks]).tolist()      # one host read per direction
    return {int(k): h / q.shape[0] for k, h in zip(ks, hits)}


def recall_at_k(imu_emb: torch.Tensor, video_emb: torch.Tensor, ks=(1, 5, 10)):
    """{'imu_to_video': {k: frac}, 'video_to_imu': {k: frac}} for paired embeddings (row i of one side is the
    positive of row i of the other): the fraction of queries whose positive is among the first k retrieved."""
    ks = tuple(int(k) for k in ks)
    if not ks or imu_emb.shape != video_emb.shape:
        raise ValueError('recall_at_k needs paired [N, d] embeddings and at least one k')
    return {'imu_to_video': _directed_recall(imu_emb, video_emb, ks),
            'video_to_imu': _directed_recall(video_emb, imu_emb, ks)}


@torch.no_grad()
def evaluate_retrieval(model, dataloader, ks=(1, 5, 10), device='cuda'):
    """recall_at_k of a `CrossModalModel`'s two projection outputs over a loader of {'imu', 'video'} batches."""
    model = model.to(device)
    was_training = model.training
    model.eval()
    try:
        a, b = [], []
        for batch in dataloader:
            ia, vb = model(batch['imu'].to(device), batch['video'].to(device))
            a.append(ia.float())
            b.append(vb.float())
    finally:
        model.train(was_training)
    return recall_at_k(torch.cat(a), torch.cat(b), ks)
