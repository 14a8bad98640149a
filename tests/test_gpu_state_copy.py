"""csrc/state_copy.hip through train_ops.StateSnapshot: ONE table that holds every access path of the kernel — 16-byte lanes, dwords,
bytes, each tail, chunks of exactly 16 KiB and one byte either side, more than one block per job, 300 jobs, a zero-size tensor — packed
into the flat buffer and unpacked again, bit for bit, with canary bytes around every destination and between the slots; the refusals
(a non-dense view, stream capture).  Every tensor is a view into its own canary-filled arena, so a byte written outside it shows."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CANARY, PAD = 0xA5, 64


def _bytes(t):
    """The tensor's bytes in storage order (dense tensors only), as uint8."""
    if t.numel() == 0:
        return torch.empty(0, dtype=torch.uint8, device=t.device)
    return torch.as_strided(t, (t.numel(),), (1,)).view(torch.uint8)


class _Arena:
    """nbytes of payload at `lead` bytes past a 16-byte boundary, PAD canary bytes before and after."""

    def __init__(self, dev, gen, nbytes, lead):
        self.buf = torch.full((PAD + lead + nbytes + PAD,), CANARY, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.hi = PAD + lead, PAD + lead + nbytes
        self.fill(gen)

    def payload(self):
        return self.buf[self.lo:self.hi]

    def fill(self, gen):
        self.payload().copy_(torch.randint(0, 256, (self.hi - self.lo,), dtype=torch.uint8, generator=gen).to(self.buf.device))

    def canaries_intact(self):
        return bool((self.buf[:self.lo] == CANARY).all()) and bool((self.buf[self.hi:] == CANARY).all())


def _build(dev):
    gen = torch.Generator().manual_seed(22)
    named, arenas = [], []

    def add(name, dtype, shape, lead=0, strides=None):
        numel = 1
        for s in shape:
            numel *= s
        item = torch.empty(0, dtype=dtype).element_size()
        a = _Arena(dev, gen, numel * item, lead)
        flat = a.payload().view(dtype)
        t = flat.view(shape) if strides is None else torch.as_strided(flat, shape, strides)
        assert t.data_ptr() == a.buf.data_ptr() + a.lo
        named.append((name, t))
        arenas.append(a)

    for n in (1, 3, 4, 4095, 4096, 4097, 3 * 4096 + 5):  # 4096 fp32 = one 16 KiB chunk
        add("f32_%d" % n, torch.float32, (n,))
    add("nbt_a", torch.int64, ())
    add("nbt_b", torch.int64, ())
    for n in (1, 15, 17, 16385):
        add("u8_%d" % n, torch.uint8, (n,))
    add("bf16_7", torch.bfloat16, (7,))
    add("f32_view_one_float_in", torch.float32, (4099,), lead=4)   # the dword path, two blocks, a 3-float tail
    add("u8_view_one_byte_in", torch.uint8, (16391,), lead=1)       # the byte path, two blocks
    add("f32_dword_short", torch.float32, (2,), lead=8)
    add("weight_ndhwc", torch.float32, (8, 6, 3, 5, 5), strides=(450, 1, 150, 30, 6))  # channels_last_3d of [8, 6, 3, 5, 5]
    assert named[-1][1].is_contiguous(memory_format=torch.channels_last_3d)
    named.append(("empty", torch.empty((0, 3), dtype=torch.float32, device=dev)))
    arenas.append(None)
    for k in range(300 - sum(1 for a in arenas if a is not None)):
        add("many_%d" % k, torch.float32, (1 + (k * 7) % 61,), lead=(0, 4, 8, 12)[k % 4])
    return gen, named, arenas


@pytest.fixture(scope="module")
def case(avt, dev):
    from avtex import train_ops

    gen, named, arenas = _build(dev)
    snap = train_ops.StateSnapshot(named)
    return gen, named, arenas, snap


def test_the_table_holds_300_jobs_and_every_path(avt, dev, case):
    _, named, arenas, snap = case
    live = [t for _, t in named if t.numel()]
    assert len(live) == 300 and len(named) == 301
    assert snap._pack_tab[0].numel() == 300 * 32 and snap._unpack_tab[0].numel() == 300 * 32  # the zero-size tensor has no job
    want_blocks = sum(-(-t.numel() * t.element_size() // 16384) for t in live)
    assert snap._pack_tab[2] == snap._unpack_tab[2] == want_blocks > 300
    assert all(o % 16 == 0 for o in snap.offsets) and snap.flat.data_ptr() % 16 == 0
    ptrs = {t.data_ptr() % 16 for t in live}
    assert {0, 4, 1} <= ptrs  # 16-byte, dword and byte alignment are all in the table


def test_pack_then_unpack_is_bit_exact_and_writes_nothing_else(avt, dev, case):
    from avtex import train_ops

    gen, named, arenas, snap = case
    before = train_ops.CALLS["state_copy_multi"]
    want = [_bytes(t).cpu().clone() for _, t in named]
    h = snap.take()
    assert train_ops.CALLS["state_copy_multi"] == before + 1  # one launch
    views = h.wait()
    assert list(views) == [n for n, _ in named]
    for (name, t), w in zip(named, want):
        v = views[name]
        assert not v.is_cuda and v.dtype == t.dtype and v.shape == t.shape and v.stride() == t.stride(), name
        assert torch.equal(_bytes(v), w), name
    # the flat buffer: the slots hold the tensors, the padding between them is still zero
    flat = snap.flat.cpu()
    end = 0
    for (name, _), o, n, w in zip(named, snap.offsets, snap.nbytes, want):
        assert not flat[end:o].any(), "padding before %s" % name
        assert torch.equal(flat[o:o + n], w), name
        end = o + n
    assert not flat[end:].any()
    # the sources were only read
    assert all(torch.equal(_bytes(t).cpu(), w) for (_, t), w in zip(named, want))
    assert all(a.canaries_intact() for a in arenas if a is not None)

    # destinations perturbed, then restored from the handle's pinned buffer: one copy, one launch
    for a in arenas:
        if a is not None:
            a.fill(gen)
    assert not all(torch.equal(_bytes(t).cpu(), w) for (_, t), w in zip(named, want))
    snap.restore(h)
    assert train_ops.CALLS["state_copy_multi"] == before + 2
    torch.cuda.synchronize()
    for (name, t), w in zip(named, want):
        assert torch.equal(_bytes(t).cpu(), w), name
    assert all(a.canaries_intact() for a in arenas if a is not None)

    # ... and from loose CPU tensors that own their storage (what a loaded checkpoint holds)
    loose = {k: v.clone() for k, v in views.items()}
    h.release()
    for a in arenas:
        if a is not None:
            a.fill(gen)
    snap.restore(loose)
    torch.cuda.synchronize()
    for (name, t), w in zip(named, want):
        assert torch.equal(_bytes(t).cpu(), w), name
    assert all(a.canaries_intact() for a in arenas if a is not None)


def test_a_third_take_waits_for_the_older_buffer_and_drops_nothing(avt, dev, case):
    import threading

    gen, named, arenas, snap = case
    first = named[0][1]
    handles, seen = [], []
    for k in range(2):
        first.fill_(float(k))
        handles.append(snap.take())
    first.fill_(2.0)
    # both host buffers are owned; a host thread reads the older snapshot and releases it, as the checkpoint writer does
    def consume():
        try:
            seen.append(float(handles[0].wait()[named[0][0]][0]))
        finally:
            handles[0].release()

    t = threading.Thread(target=consume)
    t.start()
    third = snap.take()  # waits for that release
    t.join()
    assert seen == [0.0]
    assert float(handles[1].wait()[named[0][0]][0]) == 1.0 and float(third.wait()[named[0][0]][0]) == 2.0
    assert third._slot == handles[0]._slot != handles[1]._slot
    with pytest.raises(avt._lib.AvtError, match="after release"):
        handles[0].wait()
    handles[1].release()
    third.release()


def test_a_non_dense_view_and_a_host_tensor_are_refused(avt, dev):
    from avtex import train_ops

    x = torch.zeros(8, 8, device=dev)
    with pytest.raises(avt._lib.AvtError, match="not dense in storage order"):
        train_ops.StateSnapshot([("ok", x), ("strided", x[:, ::2])])
    with pytest.raises(avt._lib.AvtError, match="not dense in storage order"):
        train_ops.StateSnapshot([("expanded", x[:1].expand(8, 8))])
    with pytest.raises(avt._lib.AvtError, match="device"):
        train_ops.StateSnapshot([("host", torch.zeros(4))])
    train_ops.StateSnapshot([("transposed", x.t()), ("row", x[3])])  # dense, in another order / at an offset: fine


def test_take_and_restore_raise_under_capture(avt, dev, case):
    from avtex import train_ops

    _, named, _, snap = case
    h = snap.take()
    loose = {k: v.clone() for k, v in h.wait().items()}
    h.release()
    mark = torch.zeros(1, device=dev)
    stream = torch.cuda.Stream(device=dev)
    before = train_ops.CALLS["state_copy_multi"]
    for call in (snap.take, lambda: snap.restore(loose)):
        g = torch.cuda.CUDAGraph()
        with pytest.raises(avt._lib.AvtError, match="under stream capture"):
            with torch.cuda.graph(g, stream=stream):
                mark.add_(1)  # (so that the abandoned graph is not an empty one)
                call()
    assert train_ops.CALLS["state_copy_multi"] == before
