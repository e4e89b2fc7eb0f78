"""Results must not depend on what else the GPU is doing.  Found in round 2: with the compiler's packed-fp32 code (v_pk_fma_f32 /
v_pk_add_f32) the grouped per-pixel LayerNorm kernel returned wrong group sums for some pixels whenever ANOTHER stream kept the GPU busy
(35-40 % of its launches; never when alone) - the training step was timing-dependent, and running the decoder's weight gradients on
the side stream made the encoder's gradients nondeterministic.  pointwise.hip is built without packed-fp32 code since
(csrc/Makefile); these tests keep it that way: one launch and the whole step are repeated beside a GEMM + a streaming kernel on a
second stream and must repeat bit for bit."""
import pytest
import torch

import usseg_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


class _Load:
    """An unrelated stream of MFMA + HBM work (own tensors, own stream)."""

    def __init__(self):
        self.s = torch.cuda.Stream()
        self.a = torch.randn(2048, 2048, device=DEV, dtype=torch.bfloat16)
        self.big = torch.empty(32 << 20, device=DEV)

    def kick(self, n=4):
        with torch.cuda.stream(self.s):
            for _ in range(n):
                self.c = self.a @ self.a
                self.big.add_(1.0)


@pytest.mark.parametrize("C,G", [(30, 3), (24, 3), (32, 1), (87, 3)])
def test_grouped_layernorm_under_foreign_load(C, G):
    from ultrasound_modeling_amd import ops
    torch.manual_seed(C)
    Cp = (C + 7) // 8 * 8
    x = torch.zeros(16, 128, 128, Cp, dtype=torch.bfloat16, device=DEV)
    x[..., :C] = torch.randn(16, 128, 128, C, device=DEV).to(torch.bfloat16)
    gamma, beta = (1 + 0.1 * torch.randn(C, device=DEV)).float(), (0.1 * torch.randn(C, device=DEV)).float()
    dy = torch.zeros_like(x)
    dy[..., :C] = torch.randn(16, 128, 128, C, device=DEV).to(torch.bfloat16)

    def run():
        y = ops.norm_act_fwd(x, C, gamma, beta, torch.empty_like(x), 0, G, 1e-3, ops.ACT_LRELU, 0.3)
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        dx = ops.norm_act_bwd(x, dy, C, gamma, beta, torch.empty_like(x), dg, db, 0, G, 1e-3, ops.ACT_LRELU, 0.3)
        return y, dx, dg, db
    ref = [t.clone() for t in run()]
    torch.cuda.synchronize()
    load = _Load()
    for _ in range(12):
        load.kick()
        outs = [run() for _ in range(6)]
        torch.cuda.synchronize()
        for o in outs:
            for t, r, name in zip(o, ref, ("y", "dx", "dgamma", "dbeta")):
                assert torch.equal(t, r), f"{name} changed under concurrent load: {(t != r).sum().item()} elements"


def test_training_step_under_foreign_load():
    """Arch B at the bench size, learning rate 0 (every step has identical inputs): gradients and probabilities must repeat bit for bit
    while a second stream keeps the GPU busy - HIP-graph replay, i.e. with the decoder's weight gradients on the side stream (in line
    on the main stream where GPU_MAX_HW_QUEUES is below 3: ops._Side.fork)."""
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    net = VisionTransformer(batch_size=16, img_size=(256, 256), in_channels=1, seed=0, learning_rate=0.0)
    x, y = O.synthetic_batch(16, 256, 256, 1, seed=40)
    x, y = x.to(DEV), y.float().to(DEV)
    net.capture_graph(x, y)
    load = _Load()
    ref = None
    for i in range(16):
        load.kick(6)
        loss, probs = net.train_step(x, y)
        torch.cuda.synchronize()
        cur = (net.flat.grad.clone(), probs.clone(), loss.clone())
        if ref is None:
            ref = cur
            continue
        assert torch.equal(cur[1], ref[1]), f"step {i}: probabilities changed under concurrent load"
        assert torch.equal(cur[0], ref[0]), f"step {i}: {(cur[0] != ref[0]).sum().item()} gradient entries changed under concurrent load"
        assert cur[2].item() == ref[2].item()


def _build(arch, B, HW):
    if arch == "B":
        from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
        return VisionTransformer(batch_size=B, img_size=(HW, HW), in_channels=1, seed=0, learning_rate=0.0)
    if arch == "T":
        from ultrasound_modeling_amd.TBI_TransUNet import VisionTransformer as TransUNet
        return TransUNet(img_size=(HW, HW), batch_size=B, in_channels=1, seed=0, learning_rate=0.0)
    if arch == "A":
        from ultrasound_modeling_amd.TBI_ResNest import ResNest
        net = ResNest(HW, HW, 1, 3, ksize=3, radix=3, kpaths=4, learning_rate=0.0, seed=0)
        net.resModel.injected_masks = [None] * 8       # the always-on dropout draws a fresh mask every step: off for the repeat test
        return net
    from ultrasound_modeling_amd.SwinTransformer import SwinTransformerModel
    return SwinTransformerModel(model_name="s", img_size=(HW, HW), patch_size=(4, 4), in_chans=1, embed_dim=96, depths=[2, 2, 6, 2],
                                num_heads=[3, 6, 12, 24], window_size=8, seed=0, learning_rate=0.0)


@pytest.mark.parametrize("arch", ["B", "A", "T", "S"])
def test_lazy_weight_gradients_equal_inline_order(arch):
    """ops.lazy_wgrads() moves weight-gradient launches to the side stream behind one fork (beside the next part of the backward pass);
    the gradients must be the bits of the single-stream in-line order, eager and under foreign load.  With GPU_MAX_HW_QUEUES below 3
    (``ops._Side.fork`` False) nothing forks: the test then compares the deferred in-line order (queued, run at the end of the block)
    with the plain in-line order, and the two-stream fork itself is not exercised."""
    from ultrasound_modeling_amd import ops
    if not ops._Side.fork:
        print("GPU_MAX_HW_QUEUES < 3: no side-stream fork; deferred in-line order vs in-line order")
    B, HW = 4, 256
    net = _build(arch, B, HW)
    x, y = O.synthetic_batch(B, HW, HW, 1, seed=41)
    x, y = x.to(DEV), y.float().to(DEV)
    if arch == "S":
        y = torch.full((B, 768), 1.0 / 768, device=DEV)
    step = (lambda: net.step(x, y, train=True)) if arch == "A" else (lambda: net.train_step(x, y))
    assert ops._LAZY, "lazy weight gradients are the default"
    load = _Load()
    grads = {}
    # the Swin encoder opens lazy_wgrads() per block behind a switch of its own (SwinTransformer._LAZY_BLOCK): off, with ops._LAZY on,
    # every weight gradient runs in line where it is queued - the same bits again
    from ultrasound_modeling_amd import SwinTransformer as ST
    block0 = ST._LAZY_BLOCK
    assert block0, "per-block lazy weight gradients are the default"
    try:
        for lazy, block in [(True, True), (False, True), (True, True)] + ([(True, False), (False, False)] if arch == "S" else []):
            ops._LAZY, ST._LAZY_BLOCK = lazy, block
            for rep in range(3):
                load.kick(4)
                step()
                torch.cuda.synchronize()
                g = net.flat.grad.clone()
                assert torch.isfinite(g).all() and g.abs().sum().item() > 0
                if "ref" not in grads:
                    grads["ref"] = g
                assert torch.equal(g, grads["ref"]), f"lazy={lazy} block={block} repeat {rep}: {(g != grads['ref']).sum().item()} gradient entries differ"
    finally:
        ops._LAZY, ST._LAZY_BLOCK = True, block0
