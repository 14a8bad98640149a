"""The weight-plane cache of the training step (weight_planes.py) on the host: one validity rule for every maker, the choice of what to
re-make, the signature.  CPU tensors through the torch route (3 input channels, or _PLANES_HIP = 0): no device calls here."""
import pytest
import torch


@pytest.fixture()
def wp(avt):
    from avtex import weight_planes

    keep, weight_planes._PLANES_HIP = weight_planes._PLANES_HIP, 0
    weight_planes.CACHE.invalidate(drop=True)
    try:
        yield weight_planes
    finally:
        weight_planes._PLANES_HIP = keep
        weight_planes.CACHE.invalidate(drop=True)


def _row_scaled(rows):
    import weight_planes_refs as R  # the numpy reference of the kernel's rows (frexp's exponent), not a second copy of the package's formula

    hi, lo, wscale = R.rows_ref(rows.detach().numpy(), R.F16)
    return R.plane_tensor(hi), R.plane_tensor(lo), torch.from_numpy(wscale)


def _plain_ref(w, transposed):
    """[8, 3, 1, 7, 7]: zero taps up to 8 channels, rows [cout][taps][cin] — or, transposed, [cin][flipped taps][cout] as bf16 planes."""
    from avtex import ops
    from avtex.fused_slowfast import split_planes

    w8 = torch.zeros(w.shape[0], 8, *w.shape[2:])
    w8[:, :3] = w.detach()
    if transposed:
        return list(split_planes(w8.flip(2, 3, 4).permute(1, 2, 3, 4, 0).reshape(8, -1), ops.X3_BF16))
    return list(_row_scaled(w8.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1)))


def _stem_ref(w, g):
    """Output frame j of g as channels [j * C, (j + 1) * C) over frame taps j .. j + kt - 1; column tap k in slot k + 1 of 8, 3 of 4 channels."""
    from avtex.fused_slowfast import stem_lds_image

    c, kt = w.shape[0], w.shape[2]
    rows = torch.zeros(g, c, kt + g - 1, 7, 8, 4)
    for j in range(g):
        for k in range(7):
            rows[j, :, j:j + kt, :, k + 1, :3] = w.detach()[:, :, :, :, k].permute(0, 2, 3, 1)
    hi, lo, inv = _row_scaled(rows.reshape(g * c, -1))
    return [stem_lds_image(hi, kt + g - 1, True), stem_lds_image(lo, kt + g - 1, True), inv]


_STRIDED = dict(kernel=(1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1), grid=(1, 8, 8), out=(1, 4, 4))


def _strided_ref(w):
    """Class (rh, rw) of the input position mod 2 is reached by the taps d with (d - r - 1) % 2 == 0, descending; rows [cin][taps][cout]."""
    from avtex import ops
    from avtex.fused_slowfast import split_planes

    out = []
    for rh in range(2):
        for rw in range(2):
            dh, dw = ([d for d in (2, 1, 0) if (d - r - 1) % 2 == 0] for r in (rh, rw))
            sub = w.detach()[:, :, :, dh][:, :, :, :, dw]
            out += list(split_planes(sub.permute(1, 2, 3, 4, 0).reshape(w.shape[1], -1), ops.X3_BF16))
    return out


def _tensors(v, out):
    if torch.is_tensor(v):
        out.append(v)
    elif isinstance(v, (tuple, list)):
        for e in v:
            _tensors(e, out)
    return out


_KINDS = {
    "plain": ((8, 3, 1, 7, 7), lambda wp, w: wp._weight_planes(w, False), lambda w: _plain_ref(w, False)),
    "transposed": ((8, 3, 1, 7, 7), lambda wp, w: wp._weight_planes(w, True), lambda w: _plain_ref(w, True)),
    "stem": ((8, 3, 1, 7, 7), lambda wp, w: wp._stem_weight_image(w, 4), lambda w: _stem_ref(w, 4)),
    "strided": ((16, 8, 1, 3, 3), lambda wp, w: wp._strided_planes(w, **_STRIDED), _strided_ref),
}


@pytest.mark.parametrize("kind", sorted(_KINDS))
def test_every_maker_follows_the_one_validity_rule(wp, kind):
    shape, make, ref = _KINDS[kind]

    def check(value, w):
        got, want = _tensors(value, []), ref(w)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)

    torch.manual_seed(5)
    w = torch.nn.Parameter(torch.randn(shape))
    first = make(wp, w)
    assert make(wp, w) is first                      # a hit: the very same object
    check(first, w)
    with torch.no_grad():
        w.add_(0.25)                                 # the version moves
    second = make(wp, w)
    assert second is not first
    check(second, w)
    version = w._version
    w.data.mul_(1.5)                                 # an update the version does not see ...
    assert w._version == version
    wp.CACHE.invalidate()                            # ... is followed by this (train_ops.invalidate_weight_cache)
    third = make(wp, w)
    assert third is not second
    check(third, w)
    wp.CACHE.invalidate(drop=True)
    assert not wp.CACHE.entries
    # an entry outlives its owner under a key (the owner's id first) that a NEW tensor then gets: not served to it
    make(wp, w)
    (key, ent), = wp.CACHE.entries.items()
    assert key[0] == id(w)
    other = torch.nn.Parameter(torch.randn(shape))
    wp.CACHE.entries[(id(other),) + key[1:]] = wp.CACHE.entries.pop(key)
    del w
    assert ent.ref() is None
    check(make(wp, other), other)
    assert wp.CACHE.entries[(id(other),) + key[1:]] is not ent


def test_the_stem_image_is_rebuilt_after_invalidate_alone(wp):
    w = torch.nn.Parameter(torch.randn(8, 3, 1, 7, 7))
    img = wp._stem_weight_image(w, 4)
    assert wp._stem_weight_image(w, 4) is img
    wp.CACHE.invalidate()
    again = wp._stem_weight_image(w, 4)
    assert again is not img and all(torch.equal(a, b) for a, b in zip(again[:3], img[:3])) and again[3] == img[3]


def test_select_returns_what_can_be_remade_and_voids_a_recipe_that_no_longer_fits(wp):
    p = torch.nn.Parameter(torch.randn(4, 6))
    wp.CACHE.store("k", p, "planes", jobs=[{"a made-up recipe": 1}])
    ent = wp.CACHE.entries["k"]
    assert wp.CACHE.lookup("k", p) == "planes" and wp.CACHE.select(p.device) == []   # current: nothing to re-make
    with torch.no_grad():
        p.add_(1.0)
    assert wp.CACHE.select(p.device) == [(ent, p)]
    assert wp.CACHE.select(torch.device("meta")) == [] and ent.jobs                   # another device's refresh leaves it alone
    p.data = p.data.t().contiguous().t()                                              # same shape, other strides
    assert tuple(p.shape) == (4, 6) and p.stride() == (1, 4)
    assert wp.CACHE.select(p.device) == [] and ent.jobs is None
    assert wp.CACHE.lookup("k", p) is None


def test_the_signature_is_shape_stride_dtype_and_device(wp):
    sig = wp.signature
    a = torch.empty(2, 3)
    assert sig(a) == sig(torch.empty(2, 3)) == ((2, 3), (3, 1), torch.float32, torch.device("cpu"))
    assert sig(a) != sig(torch.empty(2, 3, device="meta"))
    assert sig(a) != sig(torch.empty(3, 2).t())
    assert sig(a) != sig(torch.empty(2, 3, dtype=torch.float64))
    assert sig(a) != sig(torch.empty(3, 2))


def test_the_cache_is_stale_when_empty_and_after_invalidate_and_not_in_between(wp):
    from avtex import train_ops

    assert not wp.CACHE.entries and train_ops.weight_cache_is_stale()
    w = torch.nn.Parameter(torch.randn(8, 3, 1, 7, 7))
    keep = wp._weight_planes(w, False), wp._stem_weight_image(w, 4)
    assert not train_ops.weight_cache_is_stale()
    with torch.no_grad():
        w.add_(1.0)
    assert train_ops.weight_cache_is_stale()
    wp._weight_planes(w, True)                       # ONE current entry is enough
    assert not train_ops.weight_cache_is_stale()
    train_ops.invalidate_weight_cache()
    assert train_ops.weight_cache_is_stale() and len(wp.CACHE.entries) == 3 and keep
