"""Layout route matrix (GPU): the kernels of csrc/pointwise.hip that move parameters between the fp32 Keras variables and the bf16 operand
layouts the GEMMs read, move weight gradients back, and build the BatchNorm constants - element by element.

Each case asserts WHICH kernel it launched (route_probe.routed) and compares every element of every destination with the plain-torch
restatement of tests/layout_restatement.py (itself checked on the CPU by tests/test_cpu_layout_restatement.py).  Destinations are
pre-filled with a sentinel - NaN for bf16 operands, a finite non-zero pattern for the fp32 gradients that are accumulated into - and hold
slack before and after the logical block; every position outside the restated written mask must still hold the sentinel bit for bit.
Source weights are randn / sqrt(fan-in) with values planted exactly on and one fp32 ulp off the ties of the bf16 rounding, one large negative
element and a large last element.

What is compared how:
  * packs (pack_weight_kernel, pack_weights_batched_kernel<false> grid form, <true> flat form): BITWISE against pack_ref - one fp32
    multiply by nscale[n] and one round-to-nearest-even, both exact in torch.  usseg_pack_weight takes no nscale: for a job that has one it is
    given the source multiplied beforehand in fp32 (the same single multiply), so all three entry points still meet pack_ref.
  * unpack_wgrad_kernel, unpack_wgrad_batched_kernel: with scale 1, 0.5, -2 the product is exact, a fused and an unfused multiply-add
    agree, and the result is BITWISE fp32 dst0 + scale*scratch (the fp64 sum of two fp32 values rounds to fp32 as the fp32 add does: 53 >= 2*24+2
    bits).  With scale = 1/3 the compiler may contract `*d + v` with `v = scale * scratch[..]` (pointwise.hip unpack_wgrad_kernel, the
    two lines that form v and store *d) into one fma: bound 4*U_F32*(|dst0| + |scale*scratch|) + tiny.
  * quad_bias_expand_kernel: BITWISE.  tconv_quad_unpack_kernel, quad_head_fold_kernel (kernel gradient): one fp32 add, BITWISE
    grad0 + dq[...].  quad_head_fold_kernel's and quad_bias_fold_kernel's dbias: four adds, c_f32(4)*U_F32*(|dbias0| + sum |d16|) + tiny; the two
    agree BITWISE at Np = 4 (the same expression; quad_bias_fold_kernel strides its classes by the literal 4 = the head's Np).
  * bn_fold_batched_kernel: 4*U_F32*mag + tiny with mag = |gamma|*rstd and |beta| + |mean*scale| + |scale*bias| (a handful of fp32 roundings and
    rsqrtf); exact zeros for C <= c < Cp; a pack that takes the stored scale as nscale is BITWISE pack_ref of that stored scale.
  * bn_finalize_stats_kernel: mean 4*U_F32*|sum|/M, var 4*U_F32*(sumsq/M + mean^2) and var >= 0 - at a mean/std ratio of 100 that bound is
    about 10^4 * 4*U_F32 relative to the variance: the documented cancelling regime is bounded, not accurate; the moving statistics
    4*U_F32*(|moving0|*momentum + |stat|*(1-momentum)) from the mean / var the kernel itself stored.
test_zz_worst_ratio_table prints the worst err / bound per bounded family and the file's wall time.

Routes, and the case that reaches each:
  * pack edge guards in both read orientations (one_partial_tile), no ragged edge (exact_tiles), pad columns between taps and after the last
    (ragged), the k_fast tie sK == sN (tie), block-diagonal placement with jobs sharing one dst and sT = 0 (grouped), the grid form's
    `id += gridDim.x` loop at 576 > 512 tiles and the flat form's 144 triples (stride_loop), 16 taps (tap16), nscale indexed by n (nscale);
    one table of all of them per form (mixed: the grid form's early exit of a workgroup past its job's last tile, the flat form's job
    lookup); tiles_per_block 1 and 5 (ragged last triple).  Refusals: k_off + Kk > tap_stride, T*tap_stride > Kw, njobs = 0, nblocks = 0.
  * the host side of the production route (test_model_pack_tables): the job tables Arch A, Arch B and the small Swin build themselves, read
    back from the device: footprints pairwise disjoint and inside their operand, the model's tilemap covers every tile once, flat == grid ==
    one usseg_pack_weight per job == pack_ref, everything no footprint covers exactly zero.  (Jobs whose k_off lies beyond one tap stride -
    the quad operands, the decoder's concatenated operand - reach usseg_pack_weight with that offset moved into the dst pointer: the single
    launcher refuses k_off + Kk > tap_stride, the batched forms check nothing.)
  * unpacks: one partial workgroup, past the single form's 1024-block cap (276 480 elements), both stride orders, n_off / k_off inside a
    larger scratch, accumulate 0 / 1, the block inside a larger gradient buffer; a batched table of six jobs of 35 ... 70 000 elements
    (max_elems drives the 256-block cap, the small jobs' surplus workgroups idle).  Refusals: n_off + Nn > Ncols, k_off + Kk > Mrows.
  * quad helpers: k = 3 and 4, Cin 40 of 48, Cout 3 of Np 4 and 5 of 8, past the 2048-block cap (k = 4, Cout 256, Cin 136); bias expand where
    4*Np exceeds one workgroup.
  * bn_fold_batched_kernel: five jobs, C = Cp, C < Cp, more than one trip of the 256-thread loop, bias NULL, eps-dominated variances.
  * bn_finalize_stats_kernel: C = 5, 256, 300 with and without moving pointers; refusal of exactly one moving pointer.
Routes no test reaches:
  * njobs >= 65536 (refused by the batched launchers: blockIdx.y) - no model builds a thousandth of that.
  * index products beyond 2^31.  unpack_wgrad_batched_kernel forms `total = T*Nn*Kk` and tconv_quad_unpack_kernel / quad_head_fold_kernel
    `total = k*k*Cout*Cin` in int: they overflow from 2^31 elements of ONE weight block (an 8 GiB fp32 gradient; k = 4: Cout*Cin >= 2^27).
    The pack kernels count 32x32 tiles in int (2^31 tiles = 2^41 elements) and index in int64; pack_weight_kernel and unpack_wgrad_kernel
    count in int64.  test_model_pack_tables prints the largest job of each model it builds and asserts that it stays below 2^31 / 64
    elements: Arch A 2^23 = 8 388 608, Arch B 1 179 648, the small Swin 16 384.  Weight blocks do not grow with the image, so Arch A and
    Arch B are at those sizes in production too, a factor 256 below the overflow.
"""
import functools
import math
import time

import pytest
import torch

import layout_restatement as LR
import usseg_oracle as O
from route_probe import TINY, U_F32, acheck, c_f32, no_launch, routed

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
T0 = time.time()
WORST = {}
BITWISE = set()
up = lambda v, m: (v + m - 1) // m * m


def chk(family, what, y, ref, mag, u, c, tiny=TINY):
    r = acheck(what, y, ref, mag, u, c, tiny=tiny)
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).reshape(-1)


def same_bits(family, what, got, want):
    """got and want hold the same bits everywhere (NaN sentinels included)."""
    BITWISE.add(family)
    assert got.dtype == want.dtype and got.numel() == want.numel(), (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = bits(got), bits(want)
    if not torch.equal(g, w):
        bad = (g != w).nonzero().reshape(-1)
        i = int(bad[0])
        pytest.fail(f"{what}: {bad.numel()} of {g.numel()} elements differ in bits; first at flat index {i}: got "
                    f"{got.reshape(-1)[i].item()!r}, want {want.reshape(-1)[i].item()!r}")


def weights(seed, n, fan_in):
    """n fp32 values: randn / sqrt(fan_in), with bf16 rounding ties and their one-ulp neighbours planted, one large negative element and a
    large last element (none of them bf16-exact)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.randn(n, device=DEV, generator=g) / math.sqrt(fan_in)
    tie = [1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23, 1 + 2.0 ** -7 + 2.0 ** -8 - 2.0 ** -23,
           1 + 2.0 ** -7 + 2.0 ** -8 + 2.0 ** -23]
    for i, v in enumerate(tie * 2):
        w[(7 + i * 7919) % n] = (-1.0 if i % 3 == 0 else 1.0) * v * 2.0 ** (i % 5 - 3)
    w[n // 2] = -1000.37
    w[n - 1] = 777.77
    return w


def free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ packs
# a spec: (src, sT, sN, sK, T, Nn, Kk, dst key, Kw, tap_stride, n_off, k_off, nscale)
def _conv_fwd(src, T, cin, cout, key, Kw=None, tap=None, n_off=0, k_off=0, nscale=None):      # Keras [k,k,Cin,Cout]: rows = out channel
    tap = tap or up(cin, 8)
    return (src, cin * cout, 1, cout, T, cout, cin, key, Kw or T * tap, tap, n_off, k_off, nscale)


def _conv_dgrad(src, T, cin, cout, key, Kw=None, tap=None):                                      # rows = in channel
    tap = tap or up(cout, 8)
    return (src, cin * cout, cout, 1, T, cin, cout, key, Kw or T * tap, tap, 0, 0, None)


@functools.lru_cache(maxsize=None)
def pack_case(name):
    """-> (specs, {dst key: elements}) of one row of the case table; sources are built once and shared by every form."""
    k = lambda s: f"{name}.{s}"
    if name == "one_partial_tile":
        return [(weights(1, 35, 7), 0, 7, 1, 1, 5, 7, k("a"), 8, 8, 0, 0, None), (weights(2, 35, 7), 0, 1, 5, 1, 5, 7, k("b"), 8, 8, 0, 0, None)]
    if name == "exact_tiles":
        return [_conv_fwd(weights(3, 9 * 64 * 32, 9 * 64), 9, 64, 32, k("f"))]
    if name == "ragged":         # Nn = cin = 40, Kk = cout = 72; tap_stride 80 > Kk, Kw = 736 > T*tap_stride
        return [_conv_dgrad(weights(4, 9 * 40 * 72, 9 * 72), 9, 40, 72, k("d"), Kw=9 * 80 + 16, tap=80)]
    if name == "tie":
        return [(weights(5, 33, 33), 0, 1, 1, 1, 1, 33, k("row"), 40, 40, 0, 0, None), (weights(6, 33, 33), 0, 1, 1, 1, 33, 1, k("col"), 8, 8, 0, 0, None)]
    if name == "grouped":        # the slab of TBI_ResNest.py pack_jobs: four branches, cin 20, cv11 16, cvkk 24
        G, cin, cv11, cvkk, T = 4, 20, 16, 24, 9
        cin_p, Up, Vp, sT = up(cin, 8), G * cv11, G * cvkk, cv11 * cvkk
        specs = []
        for g in range(G):
            k1, k2 = weights(10 + g, cin * cv11, cin), weights(20 + g, T * cv11 * cvkk, T * cv11)
            specs += [(k1, 0, 1, cv11, 1, cv11, cin, k("w1_f"), cin_p, cin_p, g * cv11, 0, None),
                      (k1, 0, cv11, 1, 1, cin, cv11, k("w1_d"), Up, Up, 0, g * cv11, None),
                      (k2, sT, 1, cvkk, T, cvkk, cv11, k("w2_f"), T * Up, Up, g * cvkk, g * cv11, None),
                      (k2, sT, cvkk, 1, T, cv11, cvkk, k("w2_d"), T * Vp, Vp, g * cv11, g * cvkk, None)]
        return specs
    if name == "stride_loop":
        return [_conv_fwd(weights(7, 9 * 256 * 256, 9 * 256), 9, 256, 256, k("f"))]
    if name == "tap16":          # Conv2DTranspose [k,k,Cout,Cin], k = 4, Cout 72, Cin 64: forward rows = out channel, dgrad rows = in channel
        w = weights(8, 16 * 72 * 64, 16 * 72)
        return [(w, 72 * 64, 64, 1, 16, 72, 64, k("f"), 16 * 64, 64, 0, 0, None), (w, 72 * 64, 1, 64, 16, 64, 72, k("d"), 16 * 72, 72, 0, 0, None)]
    if name == "nscale":         # rows placed at n_off = 8: nscale[n] and nscale[n_off + n] differ everywhere
        ns = torch.linspace(-1.5, 2.0, 48, device=DEV) ** 3 + 0.3
        ns[7] = 0.0
        assert (ns < 0).any() and (ns > 0).any() and (ns[:40] != ns[8:48]).all()
        return [_conv_fwd(weights(9, 9 * 72 * 40, 9 * 72), 9, 72, 40, k("f"), n_off=8, nscale=ns)]
    if name == "mixed":
        return [s for n in PACK_CASES[:-1] for s in pack_case(n)]
    raise KeyError(name)


PACK_CASES = ["one_partial_tile", "exact_tiles", "ragged", "tie", "grouped", "stride_loop", "tap16", "nscale", "mixed"]
SLACK = 40          # sentinel elements after the last row of every operand


def dst_sizes(specs):
    rows = {}
    for s in specs:
        rows[s[7]] = (max(rows.get(s[7], (0, 0))[0], s[10] + s[5]), s[8])
    return {key: up(r, 16) * kw + SLACK for key, (r, kw) in rows.items()}


@functools.lru_cache(maxsize=None)
def pack_expected(name):
    """{dst key: the NaN-filled operand with every job's pack_ref image laid in} - computed once per case."""
    specs = pack_case(name)
    exp = {key: torch.full((n,), NAN, dtype=BF, device=DEV) for key, n in dst_sizes(specs).items()}
    seen = {key: torch.zeros(n, dtype=torch.bool, device=DEV) for key, n in dst_sizes(specs).items()}
    for (src, sT, sN, sK, T, Nn, Kk, key, Kw, tap, n_off, k_off, ns) in specs:
        img, mask = LR.pack_ref(src, sT, sN, sK, T, Nn, Kk, (exp[key].numel(),), Kw, tap, n_off, k_off, ns)
        assert not (seen[key] & mask).any(), "two jobs of the case write one element"
        assert not torch.isnan(img.float()).any()
        exp[key][mask] = img[mask]
        seen[key] |= mask
    return exp


def premultiplied(src, sT, sN, sK, T, Nn, Kk, ns):
    """A copy of src with src[t*sT+n*sN+k*sK] *= nscale[n] (one fp32 multiply): what usseg_pack_weight, which takes no nscale, is given."""
    t, n, k = LR._tnk(T, Nn, Kk, src.device)
    idx = (t * sT + n * sN + k * sK).reshape(-1)
    out = src.clone().reshape(-1)
    out[idx] = src.reshape(-1)[idx] * ns.reshape(-1)[n.reshape(-1)]
    return out


def run_packs(specs, form, tpb=4):
    """Run the specs through one entry point into fresh NaN-filled operands -> {dst key: operand}."""
    from ultrasound_modeling_amd import ops
    dst = {key: torch.full((n,), NAN, dtype=BF, device=DEV) for key, n in dst_sizes(specs).items()}
    if form == "single":
        srcs = [s[0] if s[12] is None else premultiplied(*s[:7], s[12]) for s in specs]
        routed(lambda: [ops.pack_weight(src, *s[1:7], dst[s[7]], *s[8:12]) for src, s in zip(srcs, specs)], "pack_weight_kernel")
        return dst
    jobs = [ops.pack_job(*s[:7], dst[s[7]], *s[8:12], nscale=s[12]) for s in specs]
    table = ops.make_pack_table(jobs, DEV)
    if form == "grid":
        routed(lambda: ops.pack_weights_batched(table, len(jobs)), "pack_weights_batched_kernel<false>")
    else:
        tm = ops.make_pack_tilemap(jobs, DEV, tpb)
        for c in LR.tile_cover(jobs, tm[0].cpu()):
            assert (c == 1).all(), "the tilemap does not cover every tile once"
        routed(lambda: ops.pack_weights_batched(table, len(jobs), tm), "pack_weights_batched_kernel<true>")
    return dst


@pytest.mark.parametrize("form", ["single", "grid", "flat"])
@pytest.mark.parametrize("name", PACK_CASES)
def test_pack(name, form):
    from ultrasound_modeling_amd import ops
    specs, exp = pack_case(name), pack_expected(name)
    if name == "stride_loop":
        job = (0, 0) + specs[0][1:7] + specs[0][8:12] + (0, 0)
        assert LR.job_tiles(job) == 576 > 512 and ops.make_pack_tilemap([job], "cpu")[1] == 144
    if name == "mixed":
        assert len(specs) >= 20
    got = run_packs(specs, form)
    for key in exp:
        same_bits(f"pack ({form})", f"pack {name} {form} {key}", got[key], exp[key])
    free()


@pytest.mark.parametrize("tpb", [1, 5])
def test_pack_flat_ragged_tilemap(tpb):
    """tiles_per_block 1 (a triple per tile) and 5 (a ragged last triple for most jobs) give the bits of the default 4."""
    specs, exp = pack_case("mixed"), pack_expected("mixed")
    got = run_packs(specs, "flat", tpb)
    for key in exp:
        same_bits("pack (flat)", f"pack mixed flat tiles_per_block={tpb} {key}", got[key], exp[key])
    free()


def test_pack_refusals():
    from ultrasound_modeling_amd import ops
    src, dst = weights(1, 64, 8), torch.full((256,), NAN, dtype=BF, device=DEV)
    no_launch(lambda: ops.pack_weight(src, 0, 7, 1, 1, 5, 7, dst, 8, 8, 0, 2))          # k_off + Kk > tap_stride
    no_launch(lambda: ops.pack_weight(src, 16, 4, 1, 3, 4, 4, dst, 8, 4, 0, 0))         # T*tap_stride > Kw
    job = ops.pack_job(src, 0, 7, 1, 1, 5, 7, dst, 8, 8)
    table, tm = ops.make_pack_table([job], DEV), ops.make_pack_tilemap([job], DEV)
    no_launch(lambda: ops.pack_weights_batched(table, 0))                                # njobs = 0
    no_launch(lambda: ops.pack_weights_batched(table, 1, (tm[0], 0)))                    # nblocks = 0
    assert torch.isnan(dst.float()).all()


# ------------------------------------------------------------------------------------------------ the models' own pack tables
def _walk_cuda_tensors(root):
    """Every CUDA tensor reachable from `root` through the package's objects, modules, lists, tuples and dicts."""
    seen, out, stack = set(), [], [root]
    while stack:
        o = stack.pop()
        if id(o) in seen:
            continue
        seen.add(id(o))
        if torch.is_tensor(o):
            if o.is_cuda:
                out.append(o)
        elif isinstance(o, (list, tuple, set)):
            stack.extend(o)
        elif isinstance(o, dict):
            stack.extend(o.values())
        elif isinstance(o, torch.nn.Module) or type(o).__module__.startswith("ultrasound_modeling_amd"):
            stack.extend(getattr(o, "__dict__", {}).values())
    return out


class _Memory:
    """Typed reads of device memory by address, through the storages of the tensors a model holds."""

    def __init__(self, tensors):
        self.stores = {}
        for t in tensors:
            s = t.untyped_storage()
            self.stores[s.data_ptr()] = s
        self.bf16 = [t for t in tensors if t.dtype == BF]

    def view(self, ptr, numel, dtype):
        size = torch.empty(0, dtype=dtype).element_size()
        for base, s in self.stores.items():
            if base <= ptr and ptr + numel * size <= base + s.nbytes():
                assert (ptr - base) % size == 0
                return torch.empty(0, dtype=dtype, device=DEV).set_(s, (ptr - base) // size, (numel,))
        pytest.fail(f"{numel} x {dtype} at {ptr:#x} lie in no tensor the model holds")

    def owner(self, dst):
        own = [t for t in self.bf16 if t.data_ptr() == dst]
        assert own, f"no bf16 tensor of the model starts at the dst pointer {dst:#x}"
        return max(own, key=lambda t: t.numel())


def _model(which):
    if which == "arch_a":
        from ultrasound_modeling_amd.TBI_ResNest import ResNest
        net = ResNest(64, 64, 1, 3, ksize=3, radix=3, kpaths=4, seed=5)
        return net, net.resModel._pack_table
    if which == "arch_b":
        from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
        net = VisionTransformer(batch_size=2, img_size=(64, 64), in_channels=1, seed=3)
        net.repack()
        return net, net._pack_table
    from ultrasound_modeling_amd.SwinTransformer import SwinTransformerModel
    net = SwinTransformerModel(model_name="tiny_test", img_size=(64, 64), patch_size=(4, 4), in_chans=1, embed_dim=32, depths=[2, 2], num_heads=[2, 4],
                               window_size=4)
    net.repack()
    return net, net._pack_table


@pytest.mark.parametrize("which", ["arch_a", "arch_b", "swin"])
def test_model_pack_tables(which):
    """The descriptors a model's pack_jobs() emit, read back from the device table its repack launches with."""
    import numpy as np
    from ultrasound_modeling_amd import _lib as L
    from ultrasound_modeling_amd import ops
    net, pt = _model(which)
    table, njobs, (tm, nblocks) = pt[0], pt[1], pt[-1]
    torch.cuda.synchronize()
    jobs = [tuple(int(v) for v in row) for row in table.cpu().numpy().view(np.dtype(ops.PACK_JOB_DTYPE)).reshape(-1).tolist()]
    assert len(jobs) == njobs and tm.numel() == 3 * nblocks
    mem = _Memory(_walk_cuda_tensors(net))
    # the model's tilemap covers every tile of every job once; no job is near an int overflow
    for c in LR.tile_cover(jobs, tm.cpu()):
        assert (c == 1).all()
    biggest = max(j[LR.J_T] * j[LR.J_NN] * j[LR.J_KK] for j in jobs)
    print(f"\n  {which}: {njobs} pack jobs, {nblocks} tilemap triples, largest job {biggest} elements", end="")
    assert biggest < 2 ** 31 // 64
    # footprints: inside the operand that owns dst, pairwise disjoint (one launch writes them concurrently)
    owners, count, expect = {}, {}, {}
    for j in jobs:
        o = owners.setdefault(j[LR.J_DST], mem.owner(j[LR.J_DST]))
        assert o.is_contiguous() and o.numel() % j[LR.J_KW] == 0, (tuple(o.shape), j)
        # taps do not run into each other and the last one ends inside the row.  (usseg_pack_weight asks for more: k_off + Kk <= tap_stride and
        # T*tap_stride <= Kw.  The quad operands and the decoder's concatenated backward-data operand place a segment at a k_off beyond one tap
        # stride, which only the batched forms - they check nothing - accept.)
        assert j[LR.J_KK] <= j[LR.J_TAP] and j[LR.J_KOFF] + (j[LR.J_T] - 1) * j[LR.J_TAP] + j[LR.J_KK] <= j[LR.J_KW], j
        fp = LR.job_footprint(j, DEV)
        assert 0 <= int(fp[0]) and int(fp[-1]) < o.numel(), f"job {j} leaves its operand of {tuple(o.shape)}"
        cnt = count.setdefault(j[LR.J_DST], torch.zeros(o.numel(), dtype=torch.int32, device=DEV))
        cnt[fp] += 1
    spans = sorted((o.data_ptr(), o.data_ptr() + 2 * o.numel()) for o in owners.values())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "two packed operands overlap in memory"
    for d, cnt in count.items():
        assert int(cnt.max()) == 1, f"two jobs write one element of the operand at {d:#x}"
    # pack_ref of every job, from the fp32 masters the src pointers name
    for j in jobs:
        src = mem.view(j[LR.J_SRC], LR.job_src_extent(j), torch.float32)
        ns = mem.view(j[LR.J_NSCALE], j[LR.J_NN], torch.float32) if j[LR.J_NSCALE] else None
        o = owners[j[LR.J_DST]]
        img, mask = LR.pack_ref(src, *j[LR.J_ST:LR.J_KW], (o.numel(),), *j[LR.J_KW:LR.J_RES], ns)
        e = expect.setdefault(j[LR.J_DST], torch.zeros(o.numel(), dtype=BF, device=DEV))
        e[mask] = img[mask]

    def single():
        lib, h = L.load(), torch.cuda.current_stream().cuda_stream
        keep = []
        for j in jobs:
            sp, dp, k_off = j[LR.J_SRC], j[LR.J_DST], j[LR.J_KOFF]
            if k_off + j[LR.J_KK] > j[LR.J_TAP]:        # the same addresses with the segment's offset in the pointer: (n_off+n)*Kw + t*tap + [k_off] + k
                dp, k_off = dp + 2 * k_off, 0
            if j[LR.J_NSCALE]:
                src = mem.view(sp, LR.job_src_extent(j), torch.float32)
                keep.append(premultiplied(src, *j[LR.J_ST:LR.J_KW], mem.view(j[LR.J_NSCALE], j[LR.J_NN], torch.float32)))
                sp = keep[-1].data_ptr()
            L.check(lib.usseg_pack_weight(sp, *j[LR.J_ST:LR.J_KW], dp, j[LR.J_KW], j[LR.J_TAP], j[LR.J_NOFF], k_off, h), "pack_weight")
        torch.cuda.synchronize()

    forms = (("flat", lambda: ops.pack_weights_batched(table, njobs, (tm, nblocks)), "pack_weights_batched_kernel<true>"),
             ("grid", lambda: ops.pack_weights_batched(table, njobs), "pack_weights_batched_kernel<false>"),
             ("single", single, "pack_weight_kernel"))
    for form, fn, kernel in forms:
        for o in owners.values():
            o.zero_()                      # as on_finalize leaves them: what no job writes stays zero
        routed(fn, kernel)
        for d, o in owners.items():
            same_bits(f"pack ({form})", f"{which} {form} operand {tuple(o.shape)}", o.reshape(-1), expect[d])
            assert o.reshape(-1)[count[d] == 0].float().abs().max().item() == 0 if (count[d] == 0).any() else True
    del net
    free()


# ------------------------------------------------------------------------------------------------ unpacks
def _sentinel(n, seed):
    """A live gradient: finite, non-zero everywhere."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    v = torch.randn(n, device=DEV, generator=g)
    return torch.where(v.abs() < 1e-3, torch.full_like(v, 0.5), v)


def _unpack_geometry(T, Nn, Kk, order):
    """The logical block inside a larger [T][..][..] gradient buffer (origin (2, 3)) after 5 elements of head slack, and inside a larger
    scratch (n_off 8, k_off 3).  order 'n_fast': Keras Conv2D [tap][in][out]; 'k_fast': Conv2DTranspose [tap][out][in]."""
    n_off, k_off = 8, 3
    Mrows, Ncols = k_off + Kk + 5, n_off + Nn + 3
    NB, KB = Nn + 7, Kk + 4
    if order == "n_fast":
        sT, sN, sK = KB * NB, 1, NB
        base = 5 + 2 * NB + 3
    else:
        sT, sN, sK = NB * KB, KB, 1
        base = 5 + 3 * KB + 2
    return dict(Mrows=Mrows, Ncols=Ncols, n_off=n_off, k_off=k_off, sT=sT, sN=sN, sK=sK, base=base, numel=5 + T * KB * NB + 9)


def _check_unpack(what, buf, init, base, ref, mag, mask, exact):
    """buf: the whole gradient buffer after the launch; init: before; ref / mag / mask: unpack_ref from `base` on."""
    want = torch.cat([init[:base].double(), ref])
    full = torch.cat([torch.zeros(base, dtype=torch.bool, device=DEV), mask])
    if exact:
        same_bits("unpack_wgrad (power-of-two scale)", what, buf, want.float())
        return
    untouched = torch.where(full, torch.zeros_like(buf), buf), torch.where(full, torch.zeros_like(init), init)
    same_bits("unpack_wgrad outside the block", what + " outside the block", *untouched)
    chk("unpack_wgrad (scale 1/3)", what, buf, want, torch.cat([init[:base].double().abs(), mag]), U_F32, 4.0)


@pytest.mark.parametrize("order", ["n_fast", "k_fast"])
@pytest.mark.parametrize("size", [(1, 5, 7), (9, 192, 160)], ids=["one_partial_workgroup", "past_1024_blocks"])
def test_unpack_wgrad(size, order):
    from ultrasound_modeling_amd import ops
    T, Nn, Kk = size
    g = _unpack_geometry(T, Nn, Kk, order)
    assert (T * Nn * Kk > 1024 * 256) == (size[0] == 9)
    scratch = _sentinel(T * g["Mrows"] * g["Ncols"], 60)
    init = _sentinel(g["numel"], 61)
    first = True
    for scale in (1.0, 0.5, -2.0, 1.0 / 3.0):
        for acc in (True, False):
            buf = init.clone()
            call = lambda: ops.unpack_wgrad(scratch, g["Mrows"], g["Ncols"], T, Nn, Kk, g["n_off"], g["k_off"], buf[g["base"]:], g["sT"], g["sN"], g["sK"],
                                            scale, acc)
            routed(call, "unpack_wgrad_kernel") if first else call()
            first = False
            ref, mag, mask = LR.unpack_ref(scratch, g["Mrows"], g["Ncols"], T, Nn, Kk, g["n_off"], g["k_off"], init[g["base"]:], g["sT"], g["sN"], g["sK"],
                                           scale, acc)
            assert int(mask.sum()) == T * Nn * Kk
            _check_unpack(f"unpack {size} {order} scale={scale:.3g} acc={acc}", buf, init, g["base"], ref, mag, mask, scale != 1.0 / 3.0)
    free()


def test_unpack_wgrad_batched():
    """Six jobs of 35 ... 70 000 elements in one launch: max_elems = 70 000 needs 274 workgroups, the 256-block cap makes the largest job loop
    and leaves 255 of the 256 workgroups of a 35-element job idle.  Jobs 0 and 1 scatter the two diagonal blocks of one scratch into disjoint
    blocks of one gradient buffer, as the grouped slab does."""
    from ultrasound_modeling_amd import ops
    # (T, Nn, Kk, order, scale, accumulate, buffer, scratch)
    rows = [(1, 5, 7, "n_fast", 1.0, True, "shared", "s01"), (1, 5, 7, "n_fast", 1.0, True, "shared", "s01"), (9, 24, 16, "k_fast", 0.5, True, "b2", "s2"),
            (3, 9, 11, "n_fast", -2.0, False, "b3", "s3"), (9, 100, 70, "k_fast", 1.0 / 3.0, True, "b4", "s4"), (7, 100, 100, "n_fast", 1.0, True, "b5", "s5")]
    geo = [_unpack_geometry(T, Nn, Kk, o) for (T, Nn, Kk, o, *_r) in rows]
    # jobs 0 and 1: one scratch [1][14+..][10+..], blocks (k_off, n_off) = (0, 0) and (7, 5); one buffer, the second block 40 rows further
    geo[0].update(n_off=0, k_off=0, Mrows=16, Ncols=12)
    geo[1].update(n_off=5, k_off=7, Mrows=16, Ncols=12, base=geo[0]["base"] + 40 * geo[0]["sK"])
    geo[0]["numel"] = geo[1]["numel"] = geo[1]["base"] + 7 * geo[1]["sK"] + 20
    scr = {r[7]: _sentinel(r[0] * g["Mrows"] * g["Ncols"], 70 + i) for i, (r, g) in enumerate(zip(rows, geo))}
    init = {r[6]: _sentinel(g["numel"], 80 + i) for i, (r, g) in enumerate(zip(rows, geo))}
    buf = {key: v.clone() for key, v in init.items()}
    jobs = [ops.unpack_job(scr[r[7]], g["Mrows"], g["Ncols"], r[0], r[1], r[2], g["n_off"], g["k_off"], buf[r[6]][g["base"]:], g["sT"], g["sN"], g["sK"], r[4], r[5])
            for r, g in zip(rows, geo)]
    tab = ops.make_unpack_table(jobs, DEV)
    assert tab[1] == 6 and tab[2] == 70000 and min(r[0] * r[1] * r[2] for r in rows) == 35 and (tab[2] + 255) // 256 > 256
    routed(lambda: ops.unpack_wgrad_batched(tab), "unpack_wgrad_batched_kernel")
    # the shared buffer: the two jobs' references laid over each other (their masks must not meet)
    refs = [LR.unpack_ref(scr[r[7]], g["Mrows"], g["Ncols"], r[0], r[1], r[2], g["n_off"], g["k_off"], init[r[6]][g["base"]:], g["sT"], g["sN"], g["sK"], r[4], r[5])
            for r, g in zip(rows, geo)]
    want = init["shared"].double().clone()
    masks = []
    for i in (0, 1):
        ref, _, mask = refs[i]
        m = torch.cat([torch.zeros(geo[i]["base"], dtype=torch.bool, device=DEV), mask])
        want[m] = torch.cat([init["shared"][:geo[i]["base"]].double(), ref])[m]
        masks.append(m)
    assert not (masks[0] & masks[1]).any() and int(masks[0].sum()) == int(masks[1].sum()) == 35
    same_bits("unpack_wgrad_batched (power-of-two scale)", "batched unpack jobs 0 and 1", buf["shared"], want.float())
    for i in range(2, 6):
        r, g = rows[i], geo[i]
        ref, mag, mask = refs[i]
        assert int(mask.sum()) == r[0] * r[1] * r[2]
        _check_unpack(f"batched unpack job {i}", buf[r[6]], init[r[6]], g["base"], ref, mag, mask, i != 4)
    free()


def test_unpack_refusals():
    from ultrasound_modeling_amd import ops
    scratch, dst = _sentinel(9 * 16 * 16, 1), _sentinel(4096, 2)
    keep = dst.clone()
    no_launch(lambda: ops.unpack_wgrad(scratch, 16, 16, 9, 9, 8, 8, 0, dst, 72, 8, 1))      # n_off + Nn > Ncols
    no_launch(lambda: ops.unpack_wgrad(scratch, 16, 16, 9, 8, 9, 0, 8, dst, 72, 9, 1))      # k_off + Kk > Mrows
    assert torch.equal(dst, keep)


# ------------------------------------------------------------------------------------------------ quad helpers
@pytest.mark.parametrize("C,Np", [(3, 4), (5, 8), (100, 128)])
def test_quad_bias_expand(C, Np):
    from ultrasound_modeling_amd import ops
    assert (4 * Np > 256) == (Np == 128)
    bias = weights(90, max(C, 16), 1)[:C].contiguous()
    buf = torch.full((4 * Np + 8,), NAN, device=DEV)
    routed(lambda: ops.quad_bias_expand(bias, C, buf[:4 * Np]), "quad_bias_expand_kernel")
    want = torch.cat([LR.quad_bias_expand_ref(bias, C, Np), torch.full((8,), NAN, device=DEV)])
    same_bits("quad_bias_expand", f"quad_bias_expand C={C} Np={Np}", buf, want)
    assert (buf[:4 * Np].reshape(4, Np)[:, C:] == 0).all()


QUAD_CASES = [(3, 40, 48, 3, 4), (4, 40, 48, 3, 4), (3, 40, 48, 5, 8), (4, 40, 48, 5, 8), (4, 136, 136, 256, 256)]


@pytest.mark.parametrize("k,Cin,Cin_phys,Cout,Np", QUAD_CASES, ids=[f"k{c[0]}-cin{c[1]}of{c[2]}-cout{c[3]}of{c[4]}" for c in QUAD_CASES])
def test_quad_unpack_and_head_fold(k, Cin, Cin_phys, Cout, Np):
    from ultrasound_modeling_amd import ops
    n = k * k * Cout * Cin
    assert ((n + 255) // 256 > 2048) == (Cout == 256)
    dq = _sentinel(9 * Cin_phys * 4 * Np, 91)                 # pad rows, pad columns and unused taps hold values too: a wrong index shows
    d16 = _sentinel(4 * Np, 92)
    ginit, binit = _sentinel(n + 11, 93), _sentinel(Np + 5, 94)
    want = torch.cat([LR.quad_unpack_ref(dq, Cin_phys, Cin, Cout, Np, k, ginit[:n]).reshape(-1), ginit[n:].double()]).float()
    g1 = ginit.clone()
    routed(lambda: ops.tconv_quad_unpack(dq, Cin_phys, Cin, Cout, Np, k, g1), "tconv_quad_unpack_kernel")
    same_bits("tconv_quad_unpack", f"tconv_quad_unpack k={k} Cout={Cout}/{Np}", g1, want)
    g2, b2 = ginit.clone(), binit.clone()
    routed(lambda: ops.quad_head_fold(dq, Cin_phys, Cin, Cout, Np, k, g2, d16, b2), "quad_head_fold_kernel")
    same_bits("quad_head_fold (kernel gradient)", f"quad_head_fold k={k} Cout={Cout}/{Np}", g2, want)
    ref, mag = LR.quad_bias_fold_ref(d16, Cout, Np, binit)
    chk("quad_head_fold (dbias)", f"quad_head_fold dbias k={k} Cout={Cout}/{Np}", b2[:Cout], ref, mag, U_F32, c_f32(4))     # updated exactly once
    same_bits("quad_head_fold (dbias past Cout)", "dbias past Cout", b2[Cout:], binit[Cout:])
    if Np == 4:
        b3 = binit.clone()
        routed(lambda: ops.quad_bias_fold(d16, Cout, b3), "quad_bias_fold_kernel")
        chk("quad_bias_fold", f"quad_bias_fold C={Cout}", b3[:Cout], ref, mag, U_F32, c_f32(4))
        same_bits("quad_bias_fold == quad_head_fold dbias", "quad_bias_fold against quad_head_fold's dbias at Np = 4", b3, b2)
    free()


# ------------------------------------------------------------------------------------------------ BatchNorm constants
def test_bn_fold_batched():
    from ultrasound_modeling_amd import ops
    eps = O.KERAS["bn_eps"]
    rows = [(8, 8, True, None), (21, 24, True, None), (300, 304, True, None), (21, 24, False, None), (8, 8, True, (0.0, 1e-12))]
    P, jobs = [], []
    for i, (C, Cp, with_bias, small_var) in enumerate(rows):
        # Cp floats each, every entry a live value: what lies past C must not be read into a non-zero result
        p = {n: _sentinel(Cp, 100 + 10 * i + m) for m, n in enumerate(("gamma", "beta", "mean", "var", "bias"))}
        p["var"] = p["var"].abs() + 0.05
        if small_var:
            p["var"][0], p["var"][1] = small_var
        if not with_bias:
            p["bias"] = None
        p["scale"], p["shift"] = (torch.full((Cp + 8,), NAN, device=DEV) for _ in range(2))
        P.append(p)
        jobs.append(ops.bn_fold_job(p["gamma"], p["beta"], p["mean"], p["var"], p["bias"], p["scale"][:Cp], p["shift"][:Cp], C, eps))
    table = ops.make_bn_fold_table(jobs, DEV)
    routed(lambda: ops.bn_fold_batched(table, len(jobs)), "bn_fold_batched_kernel")
    for i, ((C, Cp, _, _), p) in enumerate(zip(rows, P)):
        sc, sh, scm, shm = LR.bn_fold_ref(p["gamma"], p["beta"], p["mean"], p["var"], p["bias"], C, Cp, eps)
        chk("bn_fold scale", f"bn_fold job {i} scale", p["scale"][:Cp], sc, scm, U_F32, 4.0)
        chk("bn_fold shift", f"bn_fold job {i} shift", p["shift"][:Cp], sh, shm, U_F32, 4.0)
        for out in (p["scale"], p["shift"]):
            same_bits("bn_fold pads", f"bn_fold job {i} pad entries", out[C:Cp], torch.zeros(Cp - C, device=DEV))
            assert torch.isnan(out[Cp:]).all(), f"bn_fold job {i} wrote past Cp"
    # nscale end to end: the stored scale of job 1 (C = 21), multiplied into a 3x3 forward operand by the pack
    ns = P[1]["scale"][:24]
    src = weights(95, 9 * 16 * 21, 9 * 16)
    spec = _conv_fwd(src, 9, 16, 21, "fold", nscale=ns)
    want, mask = LR.pack_ref(*spec[:7], (dst_sizes([spec])["fold"],), *spec[8:12], ns)
    want = torch.where(mask, want, torch.full_like(want, NAN))
    for form in ("grid", "flat", "single"):
        same_bits(f"pack ({form})", f"bn_fold -> pack with nscale, {form}", run_packs([spec], form)["fold"], want)
    free()


@pytest.mark.parametrize("moving", [True, False], ids=["moving", "no_moving"])
@pytest.mark.parametrize("C", [5, 256, 300])
def test_bn_finalize_stats(C, moving):
    from ultrasound_modeling_amd import ops
    B, H, W, Cp, mom = 2, 16, 15, up(C, 8), O.KERAS["bn_momentum"]
    M = B * H * W
    g = torch.Generator(device=DEV).manual_seed(110 + C)
    ratio = torch.tensor([0.0, 3.0, 100.0], device=DEV)[torch.arange(Cp, device=DEV) % 3]          # per-channel mean / std
    x = (torch.randn(B, H, W, Cp, device=DEV, generator=g) + ratio).to(BF)
    s, s2 = torch.zeros(Cp, device=DEV), torch.zeros(Cp, device=DEV)
    ops.channel_stats(x, C, s, s2)
    torch.cuda.synchronize()
    s, s2 = s[:C].contiguous(), s2[:C].contiguous()
    mean, var = torch.full((C + 8,), NAN, device=DEV), torch.full((C + 8,), NAN, device=DEV)
    mm0, mv0 = _sentinel(C + 8, 111), _sentinel(C + 8, 112).abs()
    mm, mv = (mm0.clone(), mv0.clone()) if moving else (None, None)
    routed(lambda: ops.bn_finalize_stats(s, s2, M, C, mom, mean, var, mm, mv), "bn_finalize_stats_kernel")
    r = LR.bn_finalize_ref(s, s2, M, mom, mm0[:C] if moving else None, mv0[:C] if moving else None, stored=(mean[:C], var[:C]))
    chk("bn_finalize mean", f"bn_finalize C={C} mean", mean[:C], r["mean"], r["mean_mag"], U_F32, 4.0, tiny=1e-30)
    chk("bn_finalize var", f"bn_finalize C={C} var", var[:C], r["var"], r["var_mag"], U_F32, 4.0, tiny=1e-30)
    assert (var[:C] >= 0).all()
    assert torch.isnan(mean[C:]).all() and torch.isnan(var[C:]).all()
    if moving:
        chk("bn_finalize moving mean", f"bn_finalize C={C} moving mean", mm[:C], r["mm"], r["mm_mag"], U_F32, 4.0, tiny=1e-30)
        chk("bn_finalize moving var", f"bn_finalize C={C} moving var", mv[:C], r["mv"], r["mv_mag"], U_F32, 4.0, tiny=1e-30)
        same_bits("bn_finalize past C", "moving statistics past C", torch.cat([mm[C:], mv[C:]]), torch.cat([mm0[C:], mv0[C:]]))
        no_launch(lambda: ops.bn_finalize_stats(s, s2, M, C, mom, mean, var, mm, None))           # exactly one moving pointer
        no_launch(lambda: ops.bn_finalize_stats(s, s2, M, C, mom, mean, var, None, mv))


def test_zz_worst_ratio_table():
    """Prints only (every check asserts on its own): the worst ratio per bounded family over the cases that ran before it in this process."""
    print("\n  worst ratio err / bound per bounded output:")
    for k in sorted(WORST):
        print(f"    {k:44s} {WORST[k]:.3f}")
    print("  compared bit for bit: " + "; ".join(sorted(BITWISE)))
    print(f"  wall time of this file so far: {time.time() - T0:.1f} s")
