"""The surface of the reference's tf.data ``Dataset.py`` (``Dataset(train_path, val_path, batch_size)``, ``OUTPUT_CHANNELS``,
``BATCH_SIZE``, ``preProcess``, ``label2vec``), the input of ``MainParallel.Process``.

Loading is ``Dataset_2.Dataset``'s: both ``.npy`` files resident in HBM (``train_data=`` / ``val_data=`` arrays accepted), label =
channel 0, x = channels 1..10, bMode dropped (Dataset.py:31-39).  What differs from ``Dataset_2`` is what an epoch is - the tf.data
pipeline ``from_tensor_slices(...).map(...).batch(batch_size)`` of MainParallel.py:52-57,126-127,154-155:
  * every sample appears exactly once per epoch, in file order, in global batches of ``batch_size``;
  * the final partial batch is KEPT (``.batch()`` without ``drop_remainder``); ``Dataset_2.next_train`` re-reads ``x[-1-B:-1]``;
  * a global batch of b <= B images is split over W replicas as ``MainParallel.shard_batch`` splits a full one: replica r gets the
    contiguous block ``[r*B/W, (r+1)*B/W)`` clipped to ``[0, b)`` (``replica_block``), so a short batch may leave the last replicas
    with no image (the iterators then yield ``None``).  How TF's ``experimental_distribute_dataset`` splits a partial batch is not
    pinned here (no TF to run); this rule is the one ``shard_batch`` extends to;
  * ``train_batches`` augments (``DataAugs.dataAug_batch``, one ``usseg_augment`` launch) and maps ``label2vec``, what
    MainParallel.py:52-57 maps over ``train_data`` each epoch; ``test_batches`` maps ``label2vec`` only.
Every replica draws the augmentation parameters of the WHOLE global batch (one ``DataAugs.draw`` per sample, in sample order, from its
own seeded ``random``) and keeps its slice: each sample gets the draw it gets in a single-process run, and the replicas' generators
never drift apart.  With ``warp=`` (``Dataset_2.Dataset``; off by default) the same holds for the warp's draws, which come from a generator of
their own, and the replica's slice is warped before it is augmented; and for the draws of ``paste=`` (lesion copy-paste, off by default), whose
lesions go into the slice before the warp.  The draws are host work; the noise is seeded from them, so the device
output is a function of the draw (and, for the noise alone, of the sample's position in the launch: ``usseg_augment`` counts pixels over the
launched batch).

``next_train`` / ``next_test`` are still ``Dataset_2``'s (the MainNumpy driver's batch provider).
"""
from __future__ import annotations

import random
from typing import Iterator, List, Optional, Tuple

import torch

from . import ops
from . import Dataset_2
from .DataAugs import dataAug_batch, draw


def replica_block(n: int, batch_size: int, rank: int, world: int) -> Tuple[int, int]:
    """[lo, hi) of replica ``rank``'s images in a global batch of ``n <= batch_size`` images (``shard_batch`` extended to a short batch;
    ``lo == hi`` when the replica holds none)."""
    assert batch_size % world == 0, "global batch must divide evenly over the replicas"
    assert 0 <= rank < world and 0 <= n <= batch_size
    per = batch_size // world
    return min(rank * per, n), min((rank + 1) * per, n)


def epoch_indices(num: int, batch_size: int, rank: int = 0, world: int = 1) -> List[List[int]]:
    """The sample indices replica ``rank`` holds in each global batch of one epoch over ``num`` samples."""
    out = []
    for start in range(0, num, batch_size):
        lo, hi = replica_block(min(batch_size, num - start), batch_size, rank, world)
        out.append(list(range(start + lo, start + hi)))
    return out


class Dataset(Dataset_2.Dataset):
    """Dataset.py:5-52.  ``batch_size`` is the GLOBAL batch (``BATCH_SIZE``); the replicas' share of it is ``replica_block``."""
    draw = staticmethod(draw)

    def __init__(self, train_path=None, val_path=None, batch_size=16, *, device="cuda", train_data=None, val_data=None, warp=None, warp_seed=0,
                 paste=None, paste_seed=0):
        print("\nInitializing Dataset...")
        self.OUTPUT_CHANNELS = 3                                                                   # :11
        self.BATCH_SIZE = batch_size                                                               # :13
        super().__init__(train_path, val_path, num_classes=self.OUTPUT_CHANNELS, device=device, train_data=train_data, val_data=val_data,
                         warp=warp, warp_seed=warp_seed, paste=paste, paste_seed=paste_seed)
        self.shape = [self.height, self.width, self.channel]                                       # :12 ([256, 80, 10] in the reference)

    def preProcess(self, input_data):
        """Dataset.py:31-39: one on-disk sample block [..., 12] -> (x fp64 [n,H,W,10], label fp32 [n,H,W,1])."""
        input_data = torch.as_tensor(input_data)
        t_y = input_data[..., 0].to(torch.float32)
        t_x = input_data[..., 1:11].to(torch.float64)
        return t_x.reshape(-1, self.shape[0], self.shape[1], self.shape[2]), t_y.reshape(-1, self.shape[0], self.shape[1], 1)

    def label2vec(self, image, label):
        """Dataset.py:41-52 on the device: (image, label [n,H,W] or [n,H,W,1]) -> (image, soft class maps fp32 [n,H,W,3])."""
        label = torch.as_tensor(label).to(self.device, torch.float32).reshape(-1, self.shape[0], self.shape[1])
        return image, Dataset_2.label2vec(label, self.OUTPUT_CHANNELS)

    # ------------------------------------------------------------------ one epoch, this replica's part of every global batch
    def train_batches(self, rank: int = 0, world: int = 1, rng=random) -> Iterator[Tuple[Optional[torch.Tensor], Optional[torch.Tensor], int]]:
        """Yields ``(x bf16 [b_r,H,W,roundup(C,8)], y fp32 [b_r,H,W,3], b)`` per global batch of ``b`` images: the augmented slice of replica
        ``rank``, or ``(None, None, b)`` when it holds none.  The draws of all ``b`` samples are taken from ``rng`` in sample order; with ``warp``
        (``Dataset_2.Dataset``) so are the warp's, from its own generator, and the slice is warped before it is augmented; with ``paste`` the paste's,
        from a third generator, and its lesions go into the slice first."""
        B = self.BATCH_SIZE
        for start in range(0, self.num_tr, B):
            b = min(B, self.num_tr - start)
            params = [self.draw(rng) for _ in range(b)]
            pastes = self.draw_pastes(b)                    # None without paste; every replica draws all b, as for params
            warps = self.draw_warps(b)                      # None without warp; likewise
            lo, hi = replica_block(b, B, rank, world)
            if lo == hi:
                yield None, None, b
                continue
            x, y = self.x_tr[start + lo:start + hi], self.y_tr[start + lo:start + hi]
            if pastes is not None:
                x, y = self.pasted(x, y, pastes[lo:hi])
            if warps is not None:
                x, y = self.warped(x, y, warps[lo:hi])
            x, y = self._augment(x, y, params[lo:hi])
            yield x, y, b

    def test_batches(self, rank: int = 0, world: int = 1) -> Iterator[Tuple[Optional[torch.Tensor], Optional[torch.Tensor], int]]:
        """As ``train_batches`` over the validation set, with ``label2vec`` and no augmentation (Dataset.py:26-28)."""
        B = self.BATCH_SIZE
        for start in range(0, self.num_te, B):
            b = min(B, self.num_te - start)
            lo, hi = replica_block(b, B, rank, world)
            if lo == hi:
                yield None, None, b
                continue
            x, y = self._plain(self.x_te[start + lo:start + hi], self.y_te[start + lo:start + hi])
            yield x, y, b

    def _augment(self, x, y, params):
        return dataAug_batch(x, y, params=params, num_classes=self.OUTPUT_CHANNELS)

    def _plain(self, x, y):
        return ops.cast_input(x.contiguous(), ops.roundup(self.channel, 8)), Dataset_2.label2vec(y, self.OUTPUT_CHANNELS)
