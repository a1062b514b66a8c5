"""A call that overrides the pass range or the payload leaves nothing behind in the engine.

rsx_sort_from_to runs its own pass range, the mixed 8-bit + 4-bit chain runs a sort in two parts, and a flat rsx_segmented_unique
sorts the full range with or without carried positions, whatever RSX_OPT_FIRST_PASS / RSX_OPT_LAST_PASS say.  Every case here sets a
NON-default option range first and checks that the next rsx_sort_from still follows it, after calls that succeed and calls that are
refused.  Expected values are numpy's: a stable argsort of the selected key bits.  Integer work, bit-exact.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OPT_FIRST, OPT_LAST = 2, 6      # the option range of every case: bits 8..23

# name -> (n, options): the one-launch tile sort, the self-scan chain on 1024-key tiles, the plain scan-launch chain, the 8-bit chain
SHAPES = {
    "tile": (3000, {}),
    "selfscan": (70000, {}),
    "scan": (70000, {"OPT_SELF_SCAN": 0}),
    "8bit": (70000, {"OPT_RADIX_BITS": 8}),
}


@pytest.fixture(scope="module")
def mod(rsx):
    assert rsx.device_count() >= 1, "no HIP device: the product path has no CPU fallback"
    return rsx


def _order(keys, first, last):
    """Stable order by the bits of passes [first, last)."""
    field = (keys >> np.uint32(4 * first)) & np.uint32((1 << (4 * (last - first))) - 1)
    return np.argsort(field, kind="stable")


class _Case:
    """A uint32 payload engine with the option range 2..6 set, seeded keys on the device and the payload arange(n)."""

    def __init__(self, mod, torch, n, options, distinct=None):
        rng = np.random.default_rng(11)
        self.keys = rng.integers(0, 1 << 32, size=n, dtype=np.uint32)
        if distinct:
            self.keys = self.keys[:distinct][rng.integers(0, distinct, size=n)]
        self.n, self.torch = n, torch
        self.t = torch.from_numpy(self.keys.view(np.int32)).cuda()
        self.pay = torch.arange(n, dtype=torch.int32, device="cuda")
        self.e = mod.Engine("uint32", n, payload=True)
        self.e.set_stream(torch.cuda.current_stream().cuda_stream)
        for name, value in options.items():
            self.e.set_option(getattr(mod, name), value)
        self.e.set_option(mod.OPT_FIRST_PASS, OPT_FIRST)
        self.e.set_option(mod.OPT_LAST_PASS, OPT_LAST)

    def check_sort_from_to(self, first, last):
        out = self.torch.zeros(self.n, dtype=self.torch.int32, device="cuda")
        pout = self.torch.zeros(self.n, dtype=self.torch.int32, device="cuda")
        self.e.sort_from_to(self.t.data_ptr(), self.n, first, last, out.data_ptr(), self.pay.data_ptr(), pout.data_ptr())
        self.torch.cuda.synchronize()
        order = _order(self.keys, first, last)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), self.keys[order]), (first, last)
        assert np.array_equal(pout.cpu().numpy().view(np.uint32), order.astype(np.uint32)), (first, last)

    def check_sort_from_follows_the_options(self):
        self.e.sort_from(self.t.data_ptr(), self.n, self.pay.data_ptr())
        ks, ps = self.e.download(want_perm=True)
        order = _order(self.keys, OPT_FIRST, OPT_LAST)
        assert np.array_equal(ks, self.keys[order])
        assert np.array_equal(ps, order.astype(np.uint32))
        assert np.array_equal(self.t.cpu().numpy().view(np.uint32), self.keys)      # the input is never written


@pytest.mark.parametrize("shape", list(SHAPES))
def test_option_range_survives_sort_from_to(mod, shape):
    import torch
    n, options = SHAPES[shape]
    c = _Case(mod, torch, n, options)
    with c.e:
        c.check_sort_from_to(0, 8)
        c.check_sort_from_follows_the_options()


def test_mixed_chain_leaves_nothing_behind(mod):
    """Passes 0..7 with 8-bit digits: three byte passes, then the last nibble as one 4-bit pass."""
    import torch
    n, options = SHAPES["8bit"]
    c = _Case(mod, torch, n, options)
    with c.e:
        c.check_sort_from_to(0, 8)
        c.check_sort_from_follows_the_options()
        c.check_sort_from_to(0, 7)
        c.check_sort_from_follows_the_options()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_refused_call_leaves_nothing_behind(mod, shape):
    import torch
    n, options = SHAPES[shape]
    c = _Case(mod, torch, n, options)
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    pout = torch.zeros(n, dtype=torch.int32, device="cuda")
    with c.e:
        with pytest.raises(mod.RadixSortError):
            c.e.sort_from_to(c.t.data_ptr(), n, 3, 3, out.data_ptr(), c.pay.data_ptr(), pout.data_ptr())          # first == last
        c.check_sort_from_follows_the_options()
        c.check_sort_from_to(0, 8)
        with pytest.raises(mod.RadixSortError):
            c.e.sort_from_to(c.t.data_ptr(), n, 0, 8, c.t.data_ptr(), c.pay.data_ptr(), pout.data_ptr())          # output = input
        c.check_sort_from_follows_the_options()
        c.check_sort_from_to(0, 8)
    assert not out.cpu().numpy().any() and not pout.cpu().numpy().any()                                           # a refused call writes nothing


def test_keys_only_flat_sort_on_a_payload_engine(mod):
    """rsx_segmented_unique without offsets sorts the full range through the product chain: without positions it carries no payload,
    on a payload engine too; with positions it carries them.  Neither is the business of the next sort."""
    import torch
    n = 70000
    c = _Case(mod, torch, n, {}, distinct=20000)
    want_keys, want_first, want_inverse = np.unique(c.keys, return_index=True, return_inverse=True)
    kout = torch.zeros(n, dtype=torch.int32, device="cuda")
    uoff = torch.zeros(2, dtype=torch.int64, device="cuda")
    first = torch.zeros(n, dtype=torch.int32, device="cuda")
    inverse = torch.zeros(n, dtype=torch.int32, device="cuda")
    with c.e:
        c.e.segmented_unique(c.t.data_ptr(), n, None, 1, kout.data_ptr(), uoff.data_ptr())
        c.e.sync()
        assert uoff.cpu().numpy().tolist() == [0, want_keys.size]
        assert np.array_equal(kout.cpu().numpy().view(np.uint32)[:want_keys.size], want_keys)
        kout.zero_()
        uoff.zero_()
        c.e.segmented_unique(c.t.data_ptr(), n, None, 1, kout.data_ptr(), uoff.data_ptr(), d_first_out=first.data_ptr(), d_inverse_out=inverse.data_ptr())
        c.e.sync()
        assert uoff.cpu().numpy().tolist() == [0, want_keys.size]
        assert np.array_equal(kout.cpu().numpy().view(np.uint32)[:want_keys.size], want_keys)
        assert np.array_equal(first.cpu().numpy().view(np.uint32)[:want_keys.size], want_first.astype(np.uint32))
        assert np.array_equal(inverse.cpu().numpy().view(np.uint32), want_inverse.astype(np.uint32))
        c.check_sort_from_follows_the_options()
