"""What the ten calls of the segmented family answer to arguments they refuse, as one table: the status code and the call's name in
rsx_last_error() for every rule of every entry point (flags / op / kind, capacity, limits, required pointers, alignment, the buffer
rules), the special cases (the scan's in-place form, the reduction's "two inputs overlap", the unique's "keys and offsets overlap", the
payload pointers a non-payload engine ignores, the search's even-query form), and the order of the check groups where two faults meet.

A refused call launches nothing, so the buffers hold zeros and the offsets [0, N/2, N]: the few accepted rows (status 0) are either empty
inputs, which return before any launch, or tiny valid calls.  One engine of capacity 4096 per key width and payload mode."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP, N, S = 4096, 1000, 2
SLOT = 64 << 10                                      # bytes between two buffers of the arena: room for 2 * N elements of 8 bytes and for the offsets
OK, BUFFERS, CALC, RESIZE = 0, 1, 4, 7               # RSX_OK, RSX_HOST_BUFFERS_FAILED, RSX_CALCULATION_FAILED, RSX_RESIZE_FAILED
BIG = (1 << 31) + 1                                  # beyond the family's 2^31 elements
MANY = (1 << 32) - 1                                 # beyond its 2^32 - 2 segments

# argument order of the C ABI after the engine (include/radixsort_hip.h)
ORDER = {
    "sort": "d_keys d_payload n d_offsets num_segments d_keys_out d_payload_out",
    "topk": "d_keys n d_offsets num_segments k d_keys_out d_index_out",
    "select": "d_keys n d_offsets num_segments d_ranks ranks_per_segment d_keys_out d_index_out",
    "unique": "d_keys n d_offsets num_segments flags d_keys_out d_run_offsets_out d_counts_out d_first_out d_inverse_out",
    "reduce_by_key": "d_keys d_values n d_offsets num_segments flags op value_kind d_keys_out d_run_offsets_out d_values_out d_counts_out",
    "scan": "d_keys d_values n d_offsets num_segments flags op value_kind d_values_out",
    "search": "d_sorted n d_offsets num_segments d_queries num_queries d_query_offsets flags d_index_out",
    "compact": "d_keys n d_offsets num_segments d_mask d_bounds flags d_keys_out d_index_out d_kept_offsets_out",
    "merge": "d_a d_a_payload na d_a_offsets d_b d_b_payload nb d_b_offsets num_segments flags d_keys_out d_payload_out d_index_out d_out_offsets",
    "set_op": "d_a d_a_payload na d_a_offsets d_b d_b_payload nb d_b_offsets num_segments op flags d_keys_out d_payload_out d_index_out d_match_out "
              "d_out_offsets",
}
BUFFER_NAMES = ("keys keys_b pay pay_b vals off off_b ranks mask bounds queries qoff out_k out_p out_i out_m out_o out_v out_c out_f out_inv").split()


class World:
    """The buffers of one key width: an arena of zeros with valid offsets, a payload engine and a plain one, and a pointer into each
    engine's own result buffer."""

    def __init__(self, rsx, dt):
        import torch
        self.kb = np.dtype(dt).itemsize
        self.arena = torch.zeros(len(BUFFER_NAMES) * SLOT, dtype=torch.uint8, device="cuda")
        assert self.arena.data_ptr() % 256 == 0
        for i, name in enumerate(BUFFER_NAMES):
            setattr(self, name, self.arena.data_ptr() + i * SLOT)
        offsets = torch.tensor([0, N // 2, N], dtype=torch.int64, device="cuda").view(torch.uint8)
        for name in ("off", "off_b", "qoff"):
            at = BUFFER_NAMES.index(name) * SLOT
            self.arena[at:at + offsets.numel()] = offsets
        self.engines, self.owned = {}, {}
        for payload in (True, False):
            eng = rsx.Engine(dt, CAP, payload=payload)
            eng.sort_from(self.keys, N, self.pay if payload else None)          # the engine's result buffer is then one of its own
            eng.sync()
            # (asked for now: once a family call has run, the result is the caller's and rsx_result_device gives NULL)
            self.owned[payload] = eng.result_device()[0]
            assert self.owned[payload] != 0
            self.engines[payload] = eng
        self.lib = rsx.load_library()

    def own(self, payload=True):
        return self.owned[payload] + 64                                        # inside the engine's buffer, aligned to 16 bytes

    def call(self, name, args, payload=True):
        values = [args[k] for k in ORDER[name].split()]
        rc = getattr(self.lib, "rsx_segmented_" + name)(self.engines[payload]._h, *values)
        return rc, self.lib.rsx_last_error().decode()


@pytest.fixture(scope="module", params=[np.uint32, np.uint64], ids=["uint32", "uint64"])
def world(rsx, request):
    w = World(rsx, request.param)
    yield w
    for eng in w.engines.values():
        eng.sync()
        eng.close()


# Every table: (base arguments of a valid call, rows).  A row: (expected status, changed arguments[, word the message holds][, "plain": on
# the engine without payload]).  `w` is the World; +2 misaligns every element size, +4 every 8- and 16-byte rule.

def sort_table(w):
    base = dict(d_keys=w.keys, d_payload=w.pay, n=N, d_offsets=w.off, num_segments=S, d_keys_out=w.out_k, d_payload_out=w.out_p)
    return base, [
        (RESIZE, dict(n=CAP + 1)),
        (OK, dict(n=0)), (OK, dict(num_segments=0)),
        (CALC, dict(num_segments=MANY)),
        (BUFFERS, dict(d_keys=None)), (BUFFERS, dict(d_keys_out=None)), (BUFFERS, dict(d_offsets=None)),
        (BUFFERS, dict(d_payload=None)), (BUFFERS, dict(d_payload_out=None)),
        (BUFFERS, dict(d_keys=w.keys + 4)), (BUFFERS, dict(d_offsets=w.off + 4)), (BUFFERS, dict(d_payload=w.pay + 4)),
        (BUFFERS, dict(d_keys=w.own())), (BUFFERS, dict(d_offsets=w.own())), (BUFFERS, dict(d_keys_out=w.own())),
        (BUFFERS, dict(d_payload_out=w.out_k)), (BUFFERS, dict(d_payload_out=w.out_k + N * w.kb - 4)),
        (BUFFERS, dict(d_keys_out=w.keys)), (BUFFERS, dict(d_payload_out=w.off)), (BUFFERS, dict(d_keys_out=w.pay)),
        # without a payload engine the payload pointers are ignored: misaligned, on an input, on an output, inside the engine - a valid sort
        (OK, dict(d_payload=w.keys + 2, d_payload_out=w.out_k), "", "plain"),
        (OK, dict(d_payload=w.own(False), d_payload_out=w.off), "", "plain"),
        (BUFFERS, dict(d_keys_out=w.keys, d_payload=w.out_k, d_payload_out=w.out_k), "overlap", "plain"),
        # two faults: capacity or a limit before a misaligned pointer, a misaligned pointer before an overlap
        (RESIZE, dict(n=CAP + 1, d_keys=w.keys + 4)), (CALC, dict(num_segments=MANY, d_offsets=w.off + 4)),
        (BUFFERS, dict(d_offsets=w.off + 4, d_keys_out=w.keys), "aligned"),
    ]


def topk_table(w):
    base = dict(d_keys=w.keys, n=N, d_offsets=w.off, num_segments=S, k=4, d_keys_out=w.out_k, d_index_out=w.out_i)
    return base, [
        (RESIZE, dict(n=CAP + 1)),
        (OK, dict(k=0)), (OK, dict(n=0)), (OK, dict(num_segments=0)),
        (CALC, dict(k=4097)), (CALC, dict(num_segments=MANY)),
        (BUFFERS, dict(d_keys=None)), (BUFFERS, dict(d_keys_out=None)), (BUFFERS, dict(d_index_out=None)), (BUFFERS, dict(d_offsets=None)),
        (BUFFERS, dict(d_keys=w.keys + 4)), (BUFFERS, dict(d_keys_out=w.out_k + 2)), (BUFFERS, dict(d_index_out=w.out_i + 2)),
        (BUFFERS, dict(d_offsets=w.off + 4)),
        (BUFFERS, dict(d_keys=w.own())), (BUFFERS, dict(d_index_out=w.own())),
        (BUFFERS, dict(d_index_out=w.out_k)), (BUFFERS, dict(d_keys_out=w.keys)), (BUFFERS, dict(d_index_out=w.off)),
        (CALC, dict(k=4097, d_keys=w.keys + 4)), (RESIZE, dict(n=CAP + 1, d_index_out=w.out_i + 2)),
        (BUFFERS, dict(d_keys_out=w.out_k + 2, d_index_out=w.keys), "aligned"),
    ]


def select_table(w):
    base = dict(d_keys=w.keys, n=N, d_offsets=w.off, num_segments=S, d_ranks=w.ranks, ranks_per_segment=2, d_keys_out=w.out_k, d_index_out=w.out_i)
    return base, [
        (RESIZE, dict(n=CAP + 1)),
        (OK, dict(ranks_per_segment=0)), (OK, dict(n=0)), (OK, dict(num_segments=0)),
        (CALC, dict(ranks_per_segment=9)), (CALC, dict(num_segments=MANY)),
        (BUFFERS, dict(d_keys=None)), (BUFFERS, dict(d_keys_out=None)), (BUFFERS, dict(d_index_out=None)), (BUFFERS, dict(d_offsets=None)),
        (BUFFERS, dict(d_ranks=None)),
        (BUFFERS, dict(d_keys=w.keys + 4)), (BUFFERS, dict(d_keys_out=w.out_k + 2)), (BUFFERS, dict(d_index_out=w.out_i + 2)),
        (BUFFERS, dict(d_offsets=w.off + 4)), (BUFFERS, dict(d_ranks=w.ranks + 2)),
        (BUFFERS, dict(d_ranks=w.own())), (BUFFERS, dict(d_keys_out=w.own())),
        (BUFFERS, dict(d_index_out=w.out_k)), (BUFFERS, dict(d_keys_out=w.keys)), (BUFFERS, dict(d_index_out=w.ranks)), (BUFFERS, dict(d_keys_out=w.off)),
        (CALC, dict(ranks_per_segment=9, d_ranks=w.ranks + 2)), (RESIZE, dict(n=CAP + 1, d_keys=w.keys + 4)),
        (BUFFERS, dict(d_ranks=w.ranks + 2, d_index_out=w.out_k), "aligned"),
    ]


def unique_table(w):
    base = dict(d_keys=w.keys, n=N, d_offsets=w.off, num_segments=S, flags=0, d_keys_out=w.out_k, d_run_offsets_out=w.out_o, d_counts_out=w.out_c,
                d_first_out=w.out_f, d_inverse_out=w.out_inv)
    return base, [
        (CALC, dict(flags=2)), (CALC, dict(flags=1 << 31)),
        (RESIZE, dict(n=CAP + 1)),
        (OK, dict(n=0)), (OK, dict(num_segments=0)),
        (CALC, dict(num_segments=MANY)),
        (BUFFERS, dict(d_keys=None)), (BUFFERS, dict(d_keys_out=None)), (BUFFERS, dict(d_run_offsets_out=None)),
        (BUFFERS, dict(d_keys=w.keys + 4)), (BUFFERS, dict(d_keys_out=w.out_k + 2)), (BUFFERS, dict(d_run_offsets_out=w.out_o + 4)),
        (BUFFERS, dict(d_counts_out=w.out_c + 2)), (BUFFERS, dict(d_first_out=w.out_f + 2)), (BUFFERS, dict(d_inverse_out=w.out_inv + 2)),
        (BUFFERS, dict(d_offsets=w.off + 4)),
        (BUFFERS, dict(), "has_payload", "plain"), (BUFFERS, dict(d_first_out=None), "has_payload", "plain"),       # positions of a sorted call
        (BUFFERS, dict(d_keys=w.own())), (BUFFERS, dict(d_inverse_out=w.own())),
        (BUFFERS, dict(d_first_out=w.out_c)), (BUFFERS, dict(d_inverse_out=w.out_k)), (BUFFERS, dict(d_keys_out=w.keys)),
        (BUFFERS, dict(d_run_offsets_out=w.off)),
        (BUFFERS, dict(d_offsets=w.keys), "keys and offsets overlap"),
        (CALC, dict(flags=2, d_keys=w.keys + 4)), (BUFFERS, dict(d_counts_out=w.out_c + 2, d_first_out=w.out_k), "aligned"),
    ]


def reduce_table(w):
    base = dict(d_keys=w.keys, d_values=w.vals, n=N, d_offsets=w.off, num_segments=S, flags=0, op=0, value_kind=1, d_keys_out=w.out_k,
                d_run_offsets_out=w.out_o, d_values_out=w.out_v, d_counts_out=w.out_c)
    return base, [
        (CALC, dict(flags=2)), (CALC, dict(op=3)), (CALC, dict(value_kind=4)),
        (RESIZE, dict(n=CAP + 1)),
        (OK, dict(n=0)), (OK, dict(num_segments=0)),
        (CALC, dict(num_segments=MANY)),
        (BUFFERS, dict(d_keys=None)), (BUFFERS, dict(d_values=None)), (BUFFERS, dict(d_keys_out=None)), (BUFFERS, dict(d_run_offsets_out=None)),
        (BUFFERS, dict(d_values_out=None)),
        (BUFFERS, dict(d_keys=w.keys + 4)), (BUFFERS, dict(d_values=w.vals + 4)), (BUFFERS, dict(d_values=w.vals + 2, value_kind=0)),
        (BUFFERS, dict(d_keys_out=w.out_k + 2)), (BUFFERS, dict(d_run_offsets_out=w.out_o + 4)), (BUFFERS, dict(d_values_out=w.out_v + 4)),
        (BUFFERS, dict(d_counts_out=w.out_c + 2)), (BUFFERS, dict(d_offsets=w.off + 4)),
        (BUFFERS, dict(), "has_payload", "plain"),
        (BUFFERS, dict(d_values=w.own())), (BUFFERS, dict(d_counts_out=w.own())),
        (BUFFERS, dict(d_counts_out=w.out_v)), (BUFFERS, dict(d_values_out=w.vals)), (BUFFERS, dict(d_keys_out=w.off)),
        (BUFFERS, dict(d_values=w.keys), "two inputs overlap"), (BUFFERS, dict(d_offsets=w.vals), "two inputs overlap"),
        (CALC, dict(op=3, d_values=w.vals + 2)), (BUFFERS, dict(d_values_out=w.out_v + 4, d_counts_out=w.out_k), "aligned"),
    ]


def scan_table(w):
    base = dict(d_keys=w.keys, d_values=w.vals, n=N, d_offsets=w.off, num_segments=S, flags=0, op=0, value_kind=1, d_values_out=w.out_v)
    return base, [
        (CALC, dict(flags=1)), (CALC, dict(op=3)), (CALC, dict(value_kind=4)),
        (OK, dict(n=0)), (OK, dict(num_segments=0)),
        (CALC, dict(num_segments=MANY)), (CALC, dict(n=BIG)),
        (BUFFERS, dict(d_values=None)), (BUFFERS, dict(d_values_out=None)),
        (BUFFERS, dict(d_keys=w.keys + 4)), (BUFFERS, dict(d_values=w.vals + 4)), (BUFFERS, dict(d_values_out=w.out_v + 4)),
        (BUFFERS, dict(d_values=w.vals + 2, value_kind=2)), (BUFFERS, dict(d_offsets=w.off + 4)),
        (BUFFERS, dict(d_values=w.own())), (BUFFERS, dict(d_keys=w.own())), (BUFFERS, dict(d_values_out=w.own())),
        (BUFFERS, dict(d_values=w.own(), d_values_out=w.own())),                  # in place, but inside the engine
        (BUFFERS, dict(d_values_out=w.keys)), (BUFFERS, dict(d_values_out=w.off)),
        (OK, dict(d_values_out=w.vals)),                                          # in place: the one overlap that is served (a valid scan)
        (BUFFERS, dict(d_values_out=w.vals + 8), "in place"), (BUFFERS, dict(d_values_out=w.vals - 8), "in place"),
        (CALC, dict(flags=1, d_values=w.vals + 2)), (BUFFERS, dict(d_values_out=w.out_v + 4, d_values=w.keys), "aligned"),
    ]


def search_table(w):
    base = dict(d_sorted=w.keys, n=N, d_offsets=w.off, num_segments=S, d_queries=w.queries, num_queries=N, d_query_offsets=w.qoff, flags=0,
                d_index_out=w.out_i)
    return base, [
        (CALC, dict(flags=1)), (CALC, dict(d_offsets=None)),                      # (query offsets without haystack offsets)
        (OK, dict(num_queries=0)), (OK, dict(num_segments=0)),
        (CALC, dict(num_segments=MANY)), (CALC, dict(n=BIG)), (CALC, dict(num_queries=BIG)),
        (CALC, dict(d_query_offsets=None, num_queries=N + 1), "multiple"),        # the even form: num_queries / num_segments queries a segment
        (BUFFERS, dict(d_sorted=None)), (BUFFERS, dict(d_queries=None)), (BUFFERS, dict(d_index_out=None)),
        (BUFFERS, dict(d_sorted=w.keys + 4)), (BUFFERS, dict(d_queries=w.queries + 2)), (BUFFERS, dict(d_index_out=w.out_i + 2)),
        (BUFFERS, dict(d_offsets=w.off + 4)), (BUFFERS, dict(d_query_offsets=w.qoff + 4)),
        (BUFFERS, dict(d_queries=w.own())), (BUFFERS, dict(d_query_offsets=w.own())), (BUFFERS, dict(d_index_out=w.own())),
        (BUFFERS, dict(d_index_out=w.queries)), (BUFFERS, dict(d_index_out=w.keys)), (BUFFERS, dict(d_index_out=w.qoff)),
        (CALC, dict(flags=1, d_queries=w.queries + 2)), (CALC, dict(d_query_offsets=None, num_queries=N + 1, d_index_out=w.out_i + 2)),
        (BUFFERS, dict(d_index_out=w.out_i + 2, d_queries=w.keys), "aligned"),
    ]


def compact_table(w):
    base = dict(d_keys=w.keys, n=N, d_offsets=w.off, num_segments=S, d_mask=w.mask, d_bounds=None, flags=0, d_keys_out=w.out_k, d_index_out=w.out_i,
                d_kept_offsets_out=w.out_o)
    return base, [
        (CALC, dict(flags=1)), (CALC, dict(d_bounds=w.bounds)), (CALC, dict(d_mask=None)), (CALC, dict(flags=32)),       # (strict with a mask)
        (OK, dict(n=0)), (OK, dict(num_segments=0)),
        (CALC, dict(num_segments=MANY)), (CALC, dict(n=BIG)),
        (BUFFERS, dict(d_keys=None)), (BUFFERS, dict(d_kept_offsets_out=None)),
        (BUFFERS, dict(d_keys=w.keys + 4)), (BUFFERS, dict(d_keys_out=w.out_k + 2)), (BUFFERS, dict(d_index_out=w.out_i + 2)),
        (BUFFERS, dict(d_kept_offsets_out=w.out_o + 4)), (BUFFERS, dict(d_offsets=w.off + 4)), (BUFFERS, dict(d_mask=None, d_bounds=w.bounds + 2)),
        (BUFFERS, dict(d_mask=w.own())), (BUFFERS, dict(d_mask=None, d_bounds=w.own())), (BUFFERS, dict(d_kept_offsets_out=w.own())),
        (BUFFERS, dict(d_index_out=w.out_k)), (BUFFERS, dict(d_kept_offsets_out=w.out_i)),
        (BUFFERS, dict(d_keys_out=w.keys)), (BUFFERS, dict(d_index_out=w.mask)), (BUFFERS, dict(d_index_out=w.keys)),
        (BUFFERS, dict(d_mask=None, d_bounds=w.bounds, d_keys_out=None, d_index_out=w.keys)),       # the bound form reads its keys
        (OK, dict(d_keys_out=None, d_index_out=w.keys)),                          # a mask's keys are read for the key output only (a valid call)
        (CALC, dict(flags=1, d_keys=w.keys + 4)), (BUFFERS, dict(d_index_out=w.out_i + 2, d_keys_out=w.keys), "aligned"),
    ]


def merge_table(w):
    base = dict(d_a=w.keys, d_a_payload=w.pay, na=N, d_a_offsets=w.off, d_b=w.keys_b, d_b_payload=w.pay_b, nb=N, d_b_offsets=w.off_b, num_segments=S,
                flags=0, d_keys_out=w.out_k, d_payload_out=w.out_p, d_index_out=w.out_i, d_out_offsets=w.out_o)
    return base, [
        (CALC, dict(flags=1)), (CALC, dict(d_a_offsets=None)), (CALC, dict(d_b_offsets=None)),
        (CALC, dict(na=BIG)), (CALC, dict(nb=BIG)), (CALC, dict(na=1 << 30, nb=(1 << 30) + 1)), (CALC, dict(num_segments=MANY)),
        (CALC, dict(d_keys_out=None, d_payload_out=None, d_index_out=None, d_out_offsets=None, d_a_payload=None, d_b_payload=None)),
        (CALC, dict(d_a_payload=None)), (CALC, dict(d_payload_out=None)),
        (BUFFERS, dict(d_a=None)), (BUFFERS, dict(d_b=None)),
        (BUFFERS, dict(d_a=w.keys + 4)), (BUFFERS, dict(d_b=w.keys_b + 4)),
        (BUFFERS, dict(d_a_payload=w.pay + 2)), (BUFFERS, dict(d_b_payload=w.pay_b + 2)), (BUFFERS, dict(d_payload_out=w.out_p + 2)),
        (BUFFERS, dict(d_index_out=w.out_i + 2)), (BUFFERS, dict(d_keys_out=w.out_k + 2)),
        (BUFFERS, dict(d_a_offsets=w.off + 4)), (BUFFERS, dict(d_b_offsets=w.off_b + 4)), (BUFFERS, dict(d_out_offsets=w.out_o + 4)),
        (BUFFERS, dict(d_b=w.own())), (BUFFERS, dict(d_b_offsets=w.own())), (BUFFERS, dict(d_out_offsets=w.own())),
        (BUFFERS, dict(d_index_out=w.out_k)), (BUFFERS, dict(d_out_offsets=w.out_p)),
        (BUFFERS, dict(d_keys_out=w.keys)), (BUFFERS, dict(d_out_offsets=w.off_b)), (BUFFERS, dict(d_payload_out=w.pay_b)),
        (BUFFERS, dict(na=0, nb=0, d_keys_out=w.out_k + 2)),                      # empty inputs are looked at last: the pointers are still checked
        (OK, dict(na=0, nb=0)), (OK, dict(num_segments=0)), (OK, dict(na=0, nb=0, d_a_offsets=None, d_b_offsets=None)),
        (CALC, dict(flags=1, d_a=w.keys + 4)), (BUFFERS, dict(d_index_out=w.out_i + 2, d_keys_out=w.keys), "aligned"),
    ]


def set_op_table(w):
    base = dict(d_a=w.keys, d_a_payload=w.pay, na=N, d_a_offsets=w.off, d_b=w.keys_b, d_b_payload=w.pay_b, nb=N, d_b_offsets=w.off_b, num_segments=S,
                op=0, flags=0, d_keys_out=w.out_k, d_payload_out=w.out_p, d_index_out=w.out_i, d_match_out=w.out_m, d_out_offsets=w.out_o)
    return base, [
        (CALC, dict(op=4)), (CALC, dict(flags=1)), (CALC, dict(op=2)),            # (d_match_out belongs to the intersection)
        (CALC, dict(d_a_offsets=None)), (CALC, dict(d_b_offsets=None)),
        (CALC, dict(na=BIG)), (CALC, dict(nb=BIG)), (CALC, dict(na=1 << 30, nb=(1 << 30) + 1)), (CALC, dict(num_segments=MANY)),
        (CALC, dict(d_b_payload=None)), (CALC, dict(d_payload_out=None)),
        (BUFFERS, dict(d_out_offsets=None)),
        (BUFFERS, dict(d_a=None)), (BUFFERS, dict(d_b=None)),
        (BUFFERS, dict(d_a=w.keys + 4)), (BUFFERS, dict(d_b=w.keys_b + 4)),
        (BUFFERS, dict(d_a_payload=w.pay + 2)), (BUFFERS, dict(d_b_payload=w.pay_b + 2)), (BUFFERS, dict(d_payload_out=w.out_p + 2)),
        (BUFFERS, dict(d_index_out=w.out_i + 2)), (BUFFERS, dict(d_match_out=w.out_m + 2)), (BUFFERS, dict(d_keys_out=w.out_k + 2)),
        (BUFFERS, dict(d_a_offsets=w.off + 4)), (BUFFERS, dict(d_b_offsets=w.off_b + 4)), (BUFFERS, dict(d_out_offsets=w.out_o + 4)),
        (BUFFERS, dict(d_a=w.own())), (BUFFERS, dict(d_a_payload=w.own())), (BUFFERS, dict(d_match_out=w.own())),
        (BUFFERS, dict(d_match_out=w.out_i)), (BUFFERS, dict(d_out_offsets=w.out_k)),
        (BUFFERS, dict(d_keys_out=w.keys_b)), (BUFFERS, dict(d_match_out=w.pay)), (BUFFERS, dict(d_out_offsets=w.off)),
        (BUFFERS, dict(na=0, nb=0, d_keys_out=w.out_k + 2)),                      # empty inputs are looked at last
        (OK, dict(na=0, nb=0)), (OK, dict(num_segments=0)),
        (CALC, dict(op=4, d_a=w.keys + 4)), (BUFFERS, dict(d_match_out=w.out_m + 2, d_keys_out=w.keys), "aligned"),
    ]


TABLES = {"sort": sort_table, "topk": topk_table, "select": select_table, "unique": unique_table, "reduce_by_key": reduce_table, "scan": scan_table,
          "search": search_table, "compact": compact_table, "merge": merge_table, "set_op": set_op_table}


@pytest.mark.parametrize("name", list(TABLES))
def test_refused_and_accepted_arguments(world, name):
    base, rows = TABLES[name](world)
    assert world.call(name, base, payload=True)[0] == OK                          # the table's base is a valid call
    for row in rows:
        status, changed = row[0], row[1]
        word, plain = (row[2] if len(row) > 2 else ""), len(row) > 3
        rc, message = world.call(name, {**base, **changed}, payload=not plain)
        assert rc == status, (name, changed, rc, message)
        if status != OK:
            assert "rsx_segmented_" + name + ":" in message and word in message, (name, changed, message)
    # a null engine is refused by name too
    lib = world.lib
    assert getattr(lib, "rsx_segmented_" + name)(None, *[base[k] for k in ORDER[name].split()]) == CALC
    assert ("rsx_segmented_" + name + ": null engine").encode() in lib.rsx_last_error()
    for eng in world.engines.values():
        eng.sync()                                                                # the accepted rows ran on valid offsets: nothing to report
