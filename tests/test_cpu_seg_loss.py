"""``seg_loss.resolve`` on the host: every loss name has exactly one owner class, and every contradictory combination the constructor's docstring
names is refused with the text ``VisionTransformer(...)`` raises for the same arguments (the constructor calls ``resolve`` before it builds
anything, so neither needs a device)."""
import pytest

from ultrasound_modeling_amd import seg_loss as S
from ultrasound_modeling_amd.distill import Distill

TEACHER = object()          # looked at only by ``place``, on a device
OWNERS = (S.PixelLoss, S.OverlapLoss, S.LovaszLoss, S.TopkLoss, Distill)
FAMILIES = ((S.LOSSES, S.PixelLoss, {}), (S.OVERLAP_LOSSES, S.OverlapLoss, dict(overlap={})), (S.LOVASZ_LOSSES, S.LovaszLoss, {}),
            (S.TOPK_LOSSES, S.TopkLoss, {}), (S.DISTILL_LOSSES, Distill, dict(teacher=TEACHER)))


def test_every_name_resolves_to_exactly_one_owner_class():
    names = [n for tup, _, _ in FAMILIES for n in tup]
    assert len(names) == len(set(names)) == 11
    for tup, cls, kw in FAMILIES:
        for name in tup:
            own = S.resolve(name, 3, **kw)
            assert [c for c in OWNERS if isinstance(own, c)] == [cls], name
            assert own.fused_head == (cls is S.PixelLoss) and not hasattr(own, "acc")          # not placed: nothing on a device yet
            assert own.alpha == 2 and own.class_factor == [0.06329, 0.027567, 0.90914]
    assert S.resolve("cce", 3).class_loss is None and S.resolve("focal", 3).class_loss.gamma == 2.0
    assert S.resolve("dice", 3, smooth=2.0).overlap.smooth == 2.0 and S.resolve("dice", 3, overlap={}, boundary={}).boundary is not None
    tk = S.resolve("dice_topk", 3, overlap=dict(smooth=2.0))
    assert tk.overlap is None and tk.dice.smooth == 2.0 and S.resolve("topk", 3).dice is None


# the contradictions of the constructor's docstring, paragraph by paragraph
REFUSED = [
    dict(loss="nope"),
    dict(loss="cce", focal_gamma=2), dict(loss="my_loss_cat", class_factor=[1, 1]), dict(loss="focal", class_factor=[1, 1, 1, 1]),
    dict(loss="dice"), dict(loss="cce", overlap={}), dict(loss="dice", overlap={}, smooth=2.0), dict(loss="dice", alpha=0.3), dict(loss="tversky", ce_weight=1.0),
    dict(loss="dice_ce", ce_weight=0.0), dict(loss="dice", class_weight=[1, 1]), dict(loss="dice", overlap={}, class_factor=[1, 1, 1]),
    dict(loss="cce", boundary={}), dict(loss="lovasz", boundary={}), dict(loss="dice", overlap={}, boundary=dict(weight=-1.0)),
    dict(loss="cce", lovasz={}), dict(loss="lovasz", lovasz=dict(ce_weight=1.0)), dict(loss="lovasz", focal_gamma=2), dict(loss="lovasz_ce", class_factor=[1, 1, 1]),
    dict(loss="cce", topk={}), dict(loss="topk", class_factor=[1, 1, 1]), dict(loss="dice_topk", focal_gamma=2), dict(loss="topk", boundary={}),
    dict(loss="topk", lovasz={}), dict(loss="topk", overlap={}), dict(loss="dice_topk", ce_weight=1.0), dict(loss="lovasz", topk={}),
    dict(loss="distill"), dict(loss="cce", teacher=TEACHER), dict(loss="dice", overlap={}, distill={}), dict(loss="distill", teacher=TEACHER, distill=dict(temperature=9.0)),
] + [dict(loss="distill", teacher=TEACHER, **other) for other in (dict(class_factor=[1, 1, 1]), dict(focal_gamma=2), dict(overlap={}), dict(smooth=2.0), dict(boundary={}),
                                                                   dict(lovasz={}), dict(topk={}))]


def _refusal(fn, kw):
    with pytest.raises(ValueError) as e:
        fn(**kw)
    return str(e.value)


def test_resolve_refuses_what_the_constructor_refuses_with_the_same_text():
    from ultrasound_modeling_amd.TBI_TransUNet import VisionTransformer as TransUNet
    from ultrasound_modeling_amd.VisionTransformer import VisionTransformer
    for kw in REFUSED:
        kw = dict(kw)
        text = _refusal(lambda loss, **k: S.resolve(loss, 3, **k), kw)
        assert text and text == _refusal(lambda **k: VisionTransformer(2, (64, 64), 3, in_channels=1, **k), kw), kw
        assert text == _refusal(lambda **k: TransUNet((64, 64), batch_size=2, in_channels=1, **k), kw), kw
