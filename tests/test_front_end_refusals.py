"""Every refused argument of the torch wrappers, pinned: the exception class and the message of each bad call in the table below are
compared with tests/golden/front_end_refusals.json, which was recorded before the wrappers' argument handling was gathered into
radix-sort_amd/_tensor_args.py.  A row is (id, needs a device, call); rows a host tensor reaches run in the CPU suite, rows behind an
is_cuda check run on the GPU with tensors of at most 16 stored elements (the "more than 2^31" rows use a stride-0 view of one element,
refused before anything is allocated).  Two-fault rows pin which fault wins.

`python tests/test_front_end_refusals.py OUT.json` records what the rows raise with the code as it stands (all rows on a GPU machine, the
host rows elsewhere)."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "front_end_refusals.json")


class Ctx:
    """the tensors the rows share, on one device"""

    def __init__(self, torch, dev):
        t = lambda data, dtype: torch.tensor(data, dtype=dtype, device=dev)
        self.torch, self.dev = torch, dev
        self.k = t([1, 2, 3, 4, 5, 6], torch.int32)                 # sorted keys, two segments of three
        self.k64 = t([1, 2, 3, 4, 5, 6], torch.int64)
        self.kf = t([1, 2, 3, 4, 5, 6], torch.float32)
        self.h = t([1, 2, 3, 4, 5, 6], torch.float16)               # no key type, no value type
        self.k2d = self.k.reshape(2, 3)
        self.off = t([0, 3, 6], torch.int64)
        self.off32 = t([0, 3, 6], torch.int32)
        self.off2d = t([[0, 3, 6]], torch.int64)
        self.off4 = t([0, 2, 4, 6], torch.int64)
        self.v = t([1, 2, 3, 4, 5, 6], torch.float32)
        self.vi = t([1, 2, 3, 4, 5, 6], torch.int32)
        self.v5 = t([1, 2, 3, 4, 5], torch.float32)
        self.p = t([0, 1, 2, 3, 4, 5], torch.int32)
        self.pu = t([0, 1, 2, 3, 4, 5], torch.uint32)
        self.mask = t([1, 0, 1, 0, 1, 0], torch.bool)
        self.b2 = t([2, 5], torch.int32)
        self.host = torch.tensor([1, 2, 3, 4, 5, 6], dtype=torch.int32)
        self.host_off = torch.tensor([0, 3, 6], dtype=torch.int64)
        self.huge = torch.zeros(1, dtype=torch.int32, device=dev).expand((1 << 31) + 1)         # one stored element
        self.hugef = torch.zeros(1, dtype=torch.float32, device=dev).expand((1 << 31) + 1)


C, G = False, True
ROWS = [
    # -- segmented_sort, sort_rows
    ("sort.host_keys", C, lambda r, c: r.segmented_sort(c.k, c.off)),
    ("sort.host_keys_of_no_key_type", C, lambda r, c: r.segmented_sort(c.h, c.off)),
    ("sort.keys_2d", G, lambda r, c: r.segmented_sort(c.k2d, c.off)),
    ("sort.key_type", G, lambda r, c: r.segmented_sort(c.h, c.off)),
    ("sort.key_type_and_offsets", G, lambda r, c: r.segmented_sort(c.h, c.off32)),
    ("sort.offsets_dtype", G, lambda r, c: r.segmented_sort(c.k, c.off32)),
    ("sort.offsets_2d", G, lambda r, c: r.segmented_sort(c.k, c.off2d)),
    ("sort.offsets_host", G, lambda r, c: r.segmented_sort(c.k, c.host_off)),
    ("sort.payload_shape", G, lambda r, c: r.segmented_sort(c.k, c.off, c.p[:5])),
    ("sort.payload_dtype", G, lambda r, c: r.segmented_sort(c.k, c.off, c.k64)),
    ("sort.payload_host", G, lambda r, c: r.segmented_sort(c.k, c.off, c.host)),
    ("sort_rows.not_2d", C, lambda r, c: r.sort_rows(c.k)),
    ("sort_rows.too_many", C, lambda r, c: r.sort_rows(c.torch.zeros(1, 1, dtype=c.torch.int32).expand(2, (1 << 30) + 1))),
    # -- segmented_topk, topk
    ("topk.host_keys", C, lambda r, c: r.segmented_topk(c.k, c.off, 2)),
    ("topk.keys_2d", G, lambda r, c: r.segmented_topk(c.k2d, c.off, 2)),
    ("topk.key_type", G, lambda r, c: r.segmented_topk(c.h, c.off, 2)),
    ("topk.offsets_dtype", G, lambda r, c: r.segmented_topk(c.k, c.off32, 2)),
    ("topk.offsets_host", G, lambda r, c: r.segmented_topk(c.k, c.host_off, 2)),
    ("topk.k_negative", G, lambda r, c: r.segmented_topk(c.k, c.off, -1)),
    ("topk.k_large", G, lambda r, c: r.segmented_topk(c.k, c.off, 4097)),
    ("topk.key_type_and_k", G, lambda r, c: r.segmented_topk(c.h, c.off, -1)),
    ("topk_rows.host", C, lambda r, c: r.topk(c.k, 2)),
    ("topk_rows.host_of_no_key_type", C, lambda r, c: r.topk(c.h, 2)),
    ("topk_rows.dtype", G, lambda r, c: r.topk(c.h, 2)),
    ("topk_rows.k_range", G, lambda r, c: r.topk(c.k, 7)),
    # -- segmented_select, kthvalue, median, quantile
    ("select.host_keys", C, lambda r, c: r.segmented_select(c.k, c.off, c.off[:2])),
    ("select.keys_2d", G, lambda r, c: r.segmented_select(c.k2d, c.off, c.off[:2])),
    ("select.key_type", G, lambda r, c: r.segmented_select(c.h, c.off, c.off[:2])),
    ("select.offsets_dtype", G, lambda r, c: r.segmented_select(c.k, c.off32, c.off[:2])),
    ("select.offsets_2d", G, lambda r, c: r.segmented_select(c.k, c.off2d, c.off[:2])),
    ("select.ranks_float", G, lambda r, c: r.segmented_select(c.k, c.off, c.v[:2])),
    ("select.ranks_rows", G, lambda r, c: r.segmented_select(c.k, c.off, c.off)),
    ("select.ranks_host", G, lambda r, c: r.segmented_select(c.k, c.off, c.host_off[:2])),
    ("select_ranks.empty", C, lambda r, c: r.select_ranks(0)),
    ("select_ranks.k_range", C, lambda r, c: r.select_ranks(4, k=5)),
    ("select_ranks.interpolation", C, lambda r, c: r.select_ranks(4, q=c.torch.tensor([0.5]), interpolation="cubic")),
    ("kthvalue.host", C, lambda r, c: r.kthvalue(c.k, 2)),
    ("median.host", C, lambda r, c: r.median(c.k)),
    ("kthvalue.dtype", G, lambda r, c: r.kthvalue(c.h, 2)),
    ("kthvalue.k_range", G, lambda r, c: r.kthvalue(c.k, 7)),
    ("median.empty_dimension", G, lambda r, c: r.median(c.k[:0])),
    ("kthvalue.too_many", G, lambda r, c: r.kthvalue(c.torch.zeros(1, 1, dtype=c.torch.int32, device=c.dev).expand(2, (1 << 30) + 1), 1)),
    ("quantile.host", C, lambda r, c: r.quantile(c.v, 0.5)),
    ("quantile.dtype", G, lambda r, c: r.quantile(c.k, 0.5)),
    ("quantile.interpolation", G, lambda r, c: r.quantile(c.v, 0.5, interpolation="cubic")),
    ("quantile.q_2d", G, lambda r, c: r.quantile(c.v, c.torch.tensor([[0.5]]))),
    ("quantile.q_tensor_range", G, lambda r, c: r.quantile(c.v, c.torch.tensor([1.5]))),
    ("quantile.q_float_range", G, lambda r, c: r.quantile(c.v, -0.1)),
    ("quantile.q_list_range", G, lambda r, c: r.quantile(c.v, [0.5, 2.0])),
    ("quantile.empty_dimension", G, lambda r, c: r.quantile(c.v[:0], 0.5)),
    # -- segmented_unique, unique, unique_consecutive
    ("unique.keys_2d", C, lambda r, c: r.segmented_unique(c.k2d, c.off)),
    ("unique.host_keys", C, lambda r, c: r.segmented_unique(c.k, c.off)),
    ("unique.host_keys_of_no_key_type", C, lambda r, c: r.segmented_unique(c.h, c.off)),
    ("unique.offsets_none", G, lambda r, c: r.segmented_unique(c.k, None)),
    ("unique.offsets_dtype", G, lambda r, c: r.segmented_unique(c.k, c.off32)),
    ("unique.offsets_2d", G, lambda r, c: r.segmented_unique(c.k, c.off2d)),
    ("unique.offsets_host", G, lambda r, c: r.segmented_unique(c.k, c.host_off)),
    ("unique.key_type", G, lambda r, c: r.segmented_unique(c.h, c.off)),
    ("unique.too_many", G, lambda r, c: r.segmented_unique(c.huge, c.off)),
    ("unique_flat.host", C, lambda r, c: r.unique(c.k)),
    ("unique_flat.host_of_no_key_type", C, lambda r, c: r.unique_consecutive(c.h)),
    ("unique_flat.dim", C, lambda r, c: r.unique(c.k, dim=0)),
    ("unique_flat.dtype", G, lambda r, c: r.unique(c.h)),
    ("unique_consecutive.dtype", G, lambda r, c: r.unique_consecutive(c.h)),
    # -- segmented_reduce_by_key, reduce_by_key
    ("reduce_by_key.dims", C, lambda r, c: r.segmented_reduce_by_key(c.k2d, c.v, c.off)),
    ("reduce_by_key.offsets_none", C, lambda r, c: r.segmented_reduce_by_key(c.k, c.v, None)),
    ("reduce_by_key.offsets_dtype", C, lambda r, c: r.segmented_reduce_by_key(c.k, c.v, c.off32)),
    ("reduce_by_key.offsets_2d", C, lambda r, c: r.segmented_reduce_by_key(c.k, c.v, c.off2d)),
    ("reduce_by_key.offsets_host", G, lambda r, c: r.segmented_reduce_by_key(c.k, c.v, c.host_off)),
    ("reduce_by_key.op", C, lambda r, c: r.segmented_reduce_by_key(c.k, c.v, c.off, op="prod")),
    ("reduce_by_key.op_and_value_type", C, lambda r, c: r.segmented_reduce_by_key(c.k, c.h, c.off, op="prod")),
    ("reduce_by_key.op_and_key_type", C, lambda r, c: r.segmented_reduce_by_key(c.h, c.v, c.off, op="prod")),
    ("reduce_by_key.key_type", C, lambda r, c: r.segmented_reduce_by_key(c.h, c.v, c.off)),
    ("reduce_by_key.key_type_and_value_type", C, lambda r, c: r.segmented_reduce_by_key(c.h, c.h, c.off)),
    ("reduce_by_key.value_type", C, lambda r, c: r.segmented_reduce_by_key(c.k, c.h, c.off)),
    ("reduce_by_key.mean_of_integers", C, lambda r, c: r.segmented_reduce_by_key(c.k, c.vi, c.off, op="mean")),
    ("reduce_by_key.host", C, lambda r, c: r.segmented_reduce_by_key(c.k, c.v, c.off)),
    ("reduce_by_key.host_values", G, lambda r, c: r.segmented_reduce_by_key(c.k, c.v.cpu(), c.off)),
    ("reduce_by_key.shape", G, lambda r, c: r.segmented_reduce_by_key(c.k, c.v5, c.off)),
    ("reduce_by_key.too_many", G, lambda r, c: r.segmented_reduce_by_key(c.huge, c.hugef, c.off)),
    ("reduce_by_key_flat.shape", C, lambda r, c: r.reduce_by_key(c.k2d, c.v)),
    ("reduce_by_key_flat.op", C, lambda r, c: r.reduce_by_key(c.k, c.v, op="prod")),
    ("reduce_by_key_flat.host", C, lambda r, c: r.reduce_by_key(c.k, c.v)),
    ("reduce_by_key_flat.key_type", G, lambda r, c: r.reduce_by_key(c.h, c.v)),
    # -- segmented_scan, scan_by_key, cumsum
    ("scan.op", C, lambda r, c: r.segmented_scan(c.v, c.off, op="prod")),
    ("scan.op_and_value_type", C, lambda r, c: r.segmented_scan(c.h, c.off, op="prod")),
    ("scan.value_type", C, lambda r, c: r.segmented_scan(c.h, c.off)),
    ("scan.value_type_and_key_type", C, lambda r, c: r.segmented_scan(c.h, c.off, keys=c.h)),
    ("scan.key_type", C, lambda r, c: r.segmented_scan(c.v, c.off, keys=c.h)),
    ("scan.host", C, lambda r, c: r.segmented_scan(c.v, c.off)),
    ("scan.host_keys", G, lambda r, c: r.segmented_scan(c.v, c.off, keys=c.host)),
    ("scan.values_2d", G, lambda r, c: r.segmented_scan(c.v.reshape(2, 3), c.off)),
    ("scan.keys_shape", G, lambda r, c: r.segmented_scan(c.v, c.off, keys=c.k[:5])),
    ("scan.offsets_dtype", G, lambda r, c: r.segmented_scan(c.v, c.off32)),
    ("scan.offsets_2d", G, lambda r, c: r.segmented_scan(c.v, c.off2d)),
    ("scan.offsets_host", G, lambda r, c: r.segmented_scan(c.v, c.host_off)),
    ("scan.out_dtype", G, lambda r, c: r.segmented_scan(c.v, c.off, out=c.vi)),
    ("scan.out_shape", G, lambda r, c: r.segmented_scan(c.v, c.off, out=c.v5)),
    ("scan.out_strided", G, lambda r, c: r.segmented_scan(c.v[::2], None, out=c.torch.zeros(6, device=c.dev)[::2])),
    ("scan.too_many", G, lambda r, c: r.segmented_scan(c.hugef, None)),
    ("scan_by_key.shape", C, lambda r, c: r.scan_by_key(c.k2d, c.v)),
    ("scan_by_key.host", C, lambda r, c: r.scan_by_key(c.k, c.v)),
    ("scan_by_key.key_type", C, lambda r, c: r.scan_by_key(c.h, c.v)),
    ("cumsum.dtype", C, lambda r, c: r.cumsum(c.h)),
    ("cumsum.host", C, lambda r, c: r.cumsum(c.v)),
    # -- segmented_reduce, reduce_rows, amax ... max_rows
    ("segreduce.op", C, lambda r, c: r.segmented_reduce(c.v, c.off, op="prod")),
    ("segreduce.op_and_value_type", C, lambda r, c: r.segmented_reduce(c.h, c.off, op="prod")),
    ("segreduce.value_type", C, lambda r, c: r.segmented_reduce(c.h, c.off)),
    ("segreduce.mean_of_integers", C, lambda r, c: r.segmented_reduce(c.vi, c.off, op="mean")),
    ("segreduce.host", C, lambda r, c: r.segmented_reduce(c.v, c.off)),
    ("segreduce.return_index", G, lambda r, c: r.segmented_reduce(c.v, c.off, op="sum", return_index=True)),
    ("segreduce.values_2d", G, lambda r, c: r.segmented_reduce(c.v.reshape(2, 3), c.off)),
    ("segreduce.offsets_none", G, lambda r, c: r.segmented_reduce(c.v, None)),
    ("segreduce.offsets_dtype", G, lambda r, c: r.segmented_reduce(c.v, c.off32)),
    ("segreduce.offsets_2d", G, lambda r, c: r.segmented_reduce(c.v, c.off2d)),
    ("segreduce.offsets_host", G, lambda r, c: r.segmented_reduce(c.v, c.host_off)),
    ("reduce_rows.op", C, lambda r, c: r.reduce_rows(c.v, op="prod")),
    ("reduce_rows.host", C, lambda r, c: r.reduce_rows(c.v)),
    ("amax.value_type", C, lambda r, c: r.amax(c.h)),
    ("argmin.host", C, lambda r, c: r.argmin(c.v)),
    ("max_rows.host", C, lambda r, c: r.max_rows(c.v)),
    ("reduce_rows.scalar", G, lambda r, c: r.reduce_rows(c.v[0])),
    ("reduce_rows.empty_dimension", G, lambda r, c: r.reduce_rows(c.v[:0], op="max")),
    # -- segmented_expand and its conveniences
    ("expand.offsets_none", C, lambda r, c: r.segmented_expand(None)),
    ("expand.offsets_host", C, lambda r, c: r.segmented_expand(c.off, return_segment=True)),
    ("expand.offsets_dtype", G, lambda r, c: r.segmented_expand(c.off32, return_segment=True)),
    ("expand.offsets_2d", G, lambda r, c: r.segmented_expand(c.off2d, return_segment=True)),
    ("expand.n_negative", G, lambda r, c: r.segmented_expand(c.off, n=-1, return_segment=True)),
    ("expand.n_large", G, lambda r, c: r.segmented_expand(c.off, n=(1 << 31) + 1, return_segment=True)),
    ("expand.starts_without_values", G, lambda r, c: r.segmented_expand(c.off, n=6, starts=c.off[:2])),
    ("expand.starts_dtype", G, lambda r, c: r.segmented_expand(c.off, c.v, n=6, starts=c.off32[:2])),
    ("expand.starts_count", G, lambda r, c: r.segmented_expand(c.off, c.v, n=6, starts=c.off)),
    ("expand.starts_host", G, lambda r, c: r.segmented_expand(c.off, c.v, n=6, starts=c.host_off[:2])),
    ("expand.nothing_to_return", G, lambda r, c: r.segmented_expand(c.off, n=6)),
    ("expand.values_host", G, lambda r, c: r.segmented_expand(c.off, c.v.cpu()[:2], n=6)),
    ("expand.fill_count", G, lambda r, c: r.segmented_expand(c.off, c.v, n=6)),
    ("segment_ids.host", C, lambda r, c: r.segment_ids(c.off)),
    ("broadcast_segments.host", C, lambda r, c: r.broadcast_segments(c.v[:2], c.off)),
    ("broadcast_segments.count", G, lambda r, c: r.broadcast_segments(c.v, c.off, n=6)),
    ("repeat_interleave.host", C, lambda r, c: r.repeat_interleave(c.k)),
    ("repeat_interleave.lengths_float", G, lambda r, c: r.repeat_interleave(c.v)),
    ("repeat_interleave.lengths_2d", G, lambda r, c: r.repeat_interleave(c.k2d)),
    ("repeat_interleave.negative", G, lambda r, c: r.repeat_interleave(c.k, -1)),
    ("repeat_interleave.output_size", G, lambda r, c: r.repeat_interleave(c.k, 2, output_size=5)),
    ("repeat_interleave.repeats_host", G, lambda r, c: r.repeat_interleave(c.k, c.host)),
    ("repeat_interleave.repeats_count", G, lambda r, c: r.repeat_interleave(c.k, c.k[:4])),
    ("repeat_interleave.output_size_negative", G, lambda r, c: r.repeat_interleave(c.k, c.k, output_size=-1)),
    ("gather_ranges.lengths_host", C, lambda r, c: r.gather_ranges(c.v, c.off[:2], c.k[:2])),
    ("gather_ranges.starts_host", G, lambda r, c: r.gather_ranges(c.v, c.host_off[:2], c.k[:2])),
    ("gather_ranges.starts_count", G, lambda r, c: r.gather_ranges(c.v, c.off, c.k[:2])),
    ("pack_rows.host", C, lambda r, c: r.pack_rows(c.k2d, c.k[:2])),
    ("pack_rows.not_2d", G, lambda r, c: r.pack_rows(c.k, c.k[:2])),
    ("pack_rows.lengths_count", G, lambda r, c: r.pack_rows(c.k2d, c.k[:3])),
    # -- segmented_searchsorted, searchsorted, bucketize
    ("search.offsets_none", C, lambda r, c: r.segmented_searchsorted(c.k, None, c.b2)),
    ("search.values_2d", C, lambda r, c: r.segmented_searchsorted(c.k, c.off, c.k2d)),
    ("search.keys_no_tensor", C, lambda r, c: r.segmented_searchsorted([1, 2], c.off, c.b2)),
    ("search.values_no_tensor", C, lambda r, c: r.segmented_searchsorted(c.k, c.off, [1, 2])),
    ("search.key_type", C, lambda r, c: r.segmented_searchsorted(c.h, c.off, c.h[:2])),
    ("search.key_type_and_dtypes", C, lambda r, c: r.segmented_searchsorted(c.h, c.off, c.b2)),
    ("search.dtypes", C, lambda r, c: r.segmented_searchsorted(c.k, c.off, c.k64[:2])),
    ("search.host", C, lambda r, c: r.segmented_searchsorted(c.k, c.off, c.b2)),
    ("search.host_values", G, lambda r, c: r.segmented_searchsorted(c.k, c.off, c.host[:2])),
    ("search.keys_2d", G, lambda r, c: r.segmented_searchsorted(c.k2d, c.off, c.b2)),
    ("search.offsets_dtype", G, lambda r, c: r.segmented_searchsorted(c.k, c.off32, c.b2)),
    ("search.offsets_2d", G, lambda r, c: r.segmented_searchsorted(c.k, c.off2d, c.b2)),
    ("search.offsets_host", G, lambda r, c: r.segmented_searchsorted(c.k, c.host_off, c.b2)),
    ("search.value_offsets_dtype", G, lambda r, c: r.segmented_searchsorted(c.k, c.off, c.b2, value_offsets=c.off32)),
    ("search.value_offsets_host", G, lambda r, c: r.segmented_searchsorted(c.k, c.off, c.b2, value_offsets=c.host_off)),
    ("search.both_offsets_bad", G, lambda r, c: r.segmented_searchsorted(c.k, c.off32, c.b2, value_offsets=c.off32)),
    ("search.value_offsets_count", G, lambda r, c: r.segmented_searchsorted(c.k, c.off, c.b2, value_offsets=c.off4)),
    ("search.too_many", G, lambda r, c: r.segmented_searchsorted(c.huge, c.off, c.b2)),
    ("search.even_form_multiple", G, lambda r, c: r.segmented_searchsorted(c.k, c.off, c.k[:3])),
    ("searchsorted.sorter", C, lambda r, c: r.searchsorted(c.k, c.b2, sorter=c.off)),
    ("searchsorted.side", C, lambda r, c: r.searchsorted(c.k, c.b2, side="middle")),
    ("searchsorted.side_conflict", C, lambda r, c: r.searchsorted(c.k, c.b2, right=True, side="left")),
    ("searchsorted.no_tensor", C, lambda r, c: r.searchsorted([1, 2], c.b2)),
    ("searchsorted.scalar_sequence", C, lambda r, c: r.searchsorted(c.k[0], c.b2)),
    ("searchsorted.leading_dimensions", C, lambda r, c: r.searchsorted(c.k2d, c.b2)),
    ("searchsorted.host", C, lambda r, c: r.searchsorted(c.k, c.b2)),
    ("searchsorted.dtypes", C, lambda r, c: r.searchsorted(c.k, c.k64[:2])),
    ("bucketize.boundaries_2d", C, lambda r, c: r.bucketize(c.b2, c.k2d)),
    ("bucketize.key_type", C, lambda r, c: r.bucketize(c.h[:2], c.h)),
    # -- segmented_compact, masked_select, nonzero, compact_rows
    ("compact.no_tensor", C, lambda r, c: r.segmented_compact([1, 2], c.off, mask=c.mask)),
    ("compact.key_type", C, lambda r, c: r.segmented_compact(c.h, c.off, mask=c.mask)),
    ("compact.host", C, lambda r, c: r.segmented_compact(c.k, c.off, mask=c.mask)),
    ("compact.keys_2d", G, lambda r, c: r.segmented_compact(c.k2d, c.off, mask=c.mask)),
    ("compact.offsets_dtype", G, lambda r, c: r.segmented_compact(c.k, c.off32, mask=c.mask)),
    ("compact.offsets_2d", G, lambda r, c: r.segmented_compact(c.k, c.off2d, mask=c.mask)),
    ("compact.offsets_host", G, lambda r, c: r.segmented_compact(c.k, c.host_off, mask=c.mask)),
    ("compact.neither_mask_nor_bound", G, lambda r, c: r.segmented_compact(c.k, c.off)),
    ("compact.mask_and_bound", G, lambda r, c: r.segmented_compact(c.k, c.off, mask=c.mask, bound=c.b2)),
    ("compact.strict_mask", G, lambda r, c: r.segmented_compact(c.k, c.off, mask=c.mask, strict=True)),
    ("compact.mask_dtype", G, lambda r, c: r.segmented_compact(c.k, c.off, mask=c.k)),
    ("compact.mask_no_tensor", G, lambda r, c: r.segmented_compact(c.k, c.off, mask=[1, 0, 1, 0, 1, 0])),
    ("compact.mask_shape", G, lambda r, c: r.segmented_compact(c.k, c.off, mask=c.mask[:5])),
    ("compact.mask_host", G, lambda r, c: r.segmented_compact(c.k, c.off, mask=c.mask.cpu())),
    ("compact.too_many", G, lambda r, c: r.segmented_compact(c.huge, c.off, bound=c.b2)),
    ("compact.bound_dtype", G, lambda r, c: r.segmented_compact(c.k, c.off, bound=c.k64[:2])),
    ("compact.bound_no_tensor", G, lambda r, c: r.segmented_compact(c.k, c.off, bound=3)),
    ("compact.bound_count", G, lambda r, c: r.segmented_compact(c.k, c.off, bound=c.k[:3])),
    ("compact.bound_host", G, lambda r, c: r.segmented_compact(c.k, c.off, bound=c.host[:2])),
    ("masked_select.mask_dtype", C, lambda r, c: r.masked_select(c.k, c.k)),
    ("masked_select.mask_dtype_and_key_type", C, lambda r, c: r.masked_select(c.h, c.k)),
    ("masked_select.key_type", C, lambda r, c: r.masked_select(c.h, c.mask)),
    ("masked_select.host", C, lambda r, c: r.masked_select(c.k, c.mask)),
    ("masked_select.mask_host", G, lambda r, c: r.masked_select(c.k, c.mask.cpu())),
    ("nonzero.no_tensor", C, lambda r, c: r.nonzero([1, 0])),
    ("nonzero.host", C, lambda r, c: r.nonzero(c.k)),
    ("nonzero.too_many", G, lambda r, c: r.nonzero(c.huge)),
    ("compact_rows.key_type", C, lambda r, c: r.compact_rows(c.h, mask=c.mask)),
    ("compact_rows.host", C, lambda r, c: r.compact_rows(c.k2d, mask=c.mask.reshape(2, 3))),
    ("compact_rows.scalar", G, lambda r, c: r.compact_rows(c.k[0], mask=c.mask[0])),
    ("compact_rows.mask_dtype", G, lambda r, c: r.compact_rows(c.k2d, mask=c.k2d)),
    ("compact_rows.bound_no_tensor", G, lambda r, c: r.compact_rows(c.k2d, bound=3)),
    # -- segmented_histogram, bincount, bincount_rows, histc, histogram, histogram_rows
    ("histogram.no_tensor", C, lambda r, c: r.segmented_histogram([1, 2], c.off, 4)),
    ("histogram.key_type", C, lambda r, c: r.segmented_histogram(c.h, c.off, 4)),
    ("histogram.host", C, lambda r, c: r.segmented_histogram(c.k, c.off, 4)),
    ("histogram.keys_2d", G, lambda r, c: r.segmented_histogram(c.k2d, c.off, 4)),
    ("histogram.offsets_dtype", G, lambda r, c: r.segmented_histogram(c.k, c.off32, 4)),
    ("histogram.offsets_2d", G, lambda r, c: r.segmented_histogram(c.k, c.off2d, 4)),
    ("histogram.offsets_host", G, lambda r, c: r.segmented_histogram(c.k, c.host_off, 4)),
    ("histogram.edges_dtype", G, lambda r, c: r.segmented_histogram(c.k, c.off, c.k64)),
    ("histogram.edges_2d", G, lambda r, c: r.segmented_histogram(c.k, c.off, c.k2d)),
    ("histogram.edges_one", G, lambda r, c: r.segmented_histogram(c.k, c.off, c.k[:1])),
    ("histogram.edges_host", G, lambda r, c: r.segmented_histogram(c.k, c.off, c.host)),
    ("histogram.edges_too_many", G, lambda r, c: r.segmented_histogram(c.k, c.off, c.k[:1].expand(4098))),
    ("histogram.edges_with_lo", G, lambda r, c: r.segmented_histogram(c.k, c.off, c.k, lo=0)),
    ("histogram.edges_with_width_shift", G, lambda r, c: r.segmented_histogram(c.k, c.off, c.k, width_shift=1)),
    ("histogram.no_bins", G, lambda r, c: r.segmented_histogram(c.k, c.off, 0)),
    ("histogram.integer_keys_with_hi", G, lambda r, c: r.segmented_histogram(c.k, c.off, 4, hi=8)),
    ("histogram.float_keys_without_range", G, lambda r, c: r.segmented_histogram(c.kf, c.off, 4, lo=0.0)),
    ("histogram.too_many_keys", G, lambda r, c: r.segmented_histogram(c.huge, c.off, 4)),
    ("histogram.too_many_counters", G, lambda r, c: r.segmented_histogram(c.k, c.off, 1 << 31)),
    ("bincount.float", C, lambda r, c: r.bincount(c.v)),
    ("bincount.key_type", C, lambda r, c: r.bincount(c.h)),
    ("bincount.no_tensor", C, lambda r, c: r.bincount([1, 2])),
    ("bincount.host", C, lambda r, c: r.bincount(c.k)),
    ("bincount.not_1d", G, lambda r, c: r.bincount(c.k2d)),
    ("bincount.minlength", G, lambda r, c: r.bincount(c.k, minlength=-1)),
    ("bincount.negative_values", G, lambda r, c: r.bincount(c.k - 3)),
    ("bincount.too_many_bins", G, lambda r, c: r.bincount(c.k, num_bins=(1 << 31) + 1)),
    ("bincount_rows.float", C, lambda r, c: r.bincount_rows(c.v, 4)),
    ("bincount_rows.host", C, lambda r, c: r.bincount_rows(c.k2d, 4)),
    ("bincount_rows.scalar", G, lambda r, c: r.bincount_rows(c.k[0], 4)),
    ("bincount_rows.too_many_counters", G, lambda r, c: r.bincount_rows(c.k2d, 1 << 31)),
    ("histc.integer", C, lambda r, c: r.histc(c.k)),
    ("histc.host", C, lambda r, c: r.histc(c.v, bins=4, min=0, max=8)),
    ("histc.range_not_finite", G, lambda r, c: r.histc(c.v, bins=4, min=0, max=float("inf"))),
    ("histc.range_backwards", G, lambda r, c: r.histc(c.v, bins=4, min=2, max=1)),
    ("histc.no_bins", G, lambda r, c: r.histc(c.v, bins=0, min=0, max=8)),
    ("histogram_flat.edges_host", C, lambda r, c: r.histogram(c.k, c.k)),
    ("histogram_flat.integer_with_int_bins", C, lambda r, c: r.histogram(c.k, 4)),
    ("histogram_flat.range_with_edges", G, lambda r, c: r.histogram(c.k, c.k, range=(0, 8))),
    ("histogram_flat.edges_dtype", G, lambda r, c: r.histogram(c.k, c.k64)),
    ("histogram_rows.scalar", C, lambda r, c: r.histogram_rows(c.k[0], 4)),
    ("histogram_rows.host", C, lambda r, c: r.histogram_rows(c.kf.reshape(2, 3), 4, range=(0, 8))),
    ("histogram_rows.range_with_edges", G, lambda r, c: r.histogram_rows(c.k2d, c.k, range=(0, 8))),
    # -- segmented_merge, merge
    ("merge.no_tensor", C, lambda r, c: r.segmented_merge(c.k, c.off, [1, 2], c.off)),
    ("merge.key_type", C, lambda r, c: r.segmented_merge(c.h, c.off, c.h, c.off)),
    ("merge.key_type_and_dtypes", C, lambda r, c: r.segmented_merge(c.h, c.off, c.k, c.off)),
    ("merge.dtypes", C, lambda r, c: r.segmented_merge(c.k, c.off, c.k64, c.off)),
    ("merge.host", C, lambda r, c: r.segmented_merge(c.k, c.off, c.k, c.off)),
    ("merge.host_b", G, lambda r, c: r.segmented_merge(c.k, c.off, c.host, c.off)),
    ("merge.keys_2d", G, lambda r, c: r.segmented_merge(c.k2d, c.off, c.k, c.off)),
    ("merge.one_offsets", G, lambda r, c: r.segmented_merge(c.k, c.off, c.k, None)),
    ("merge.a_offsets_dtype", G, lambda r, c: r.segmented_merge(c.k, c.off32, c.k, c.off)),
    ("merge.b_offsets_2d", G, lambda r, c: r.segmented_merge(c.k, c.off, c.k, c.off2d)),
    ("merge.b_offsets_host", G, lambda r, c: r.segmented_merge(c.k, c.off, c.k, c.host_off)),
    ("merge.a_offsets_no_tensor", G, lambda r, c: r.segmented_merge(c.k, [0, 3, 6], c.k, c.off)),
    ("merge.both_offsets_bad", G, lambda r, c: r.segmented_merge(c.k, c.off32, c.k, c.off32)),
    ("merge.offsets_count", G, lambda r, c: r.segmented_merge(c.k, c.off, c.k, c.off4)),
    ("merge.one_payload", G, lambda r, c: r.segmented_merge(c.k, c.off, c.k, c.off, payload_a=c.p)),
    ("merge.payload_a_dtype", G, lambda r, c: r.segmented_merge(c.k, c.off, c.k, c.off, payload_a=c.k64, payload_b=c.p)),
    ("merge.payload_b_shape", G, lambda r, c: r.segmented_merge(c.k, c.off, c.k, c.off, payload_a=c.p, payload_b=c.p[:5])),
    ("merge.payload_b_host", G, lambda r, c: r.segmented_merge(c.k, c.off, c.k, c.off, payload_a=c.p, payload_b=c.host)),
    ("merge.payload_dtypes", G, lambda r, c: r.segmented_merge(c.k, c.off, c.k, c.off, payload_a=c.p, payload_b=c.pu)),
    ("merge.too_many", G, lambda r, c: r.segmented_merge(c.huge, None, c.k, None)),
    ("merge_rows.no_tensor", C, lambda r, c: r.merge([1, 2], c.k)),
    ("merge_rows.dimensions", C, lambda r, c: r.merge(c.k2d, c.k)),
    ("merge_rows.payload_shape", C, lambda r, c: r.merge(c.k, c.k, payload_a=c.p[:5], payload_b=c.p)),
    ("merge_rows.host", C, lambda r, c: r.merge(c.k, c.k)),
    ("merge_rows.dtypes", C, lambda r, c: r.merge(c.k2d, c.k64.reshape(2, 3))),
    # -- segmented_set_op and the four conveniences
    ("set_op.no_tensor", C, lambda r, c: r.segmented_set_op([1, 2], c.off, c.k, c.off, "union")),
    ("set_op.key_type", C, lambda r, c: r.segmented_set_op(c.h, c.off, c.h, c.off, "union")),
    ("set_op.key_type_and_op", C, lambda r, c: r.segmented_set_op(c.h, c.off, c.h, c.off, "xor")),
    ("set_op.dtypes", C, lambda r, c: r.segmented_set_op(c.k, c.off, c.k64, c.off, "union")),
    ("set_op.dtypes_and_op", C, lambda r, c: r.segmented_set_op(c.k, c.off, c.k64, c.off, "xor")),
    ("set_op.op_name", C, lambda r, c: r.segmented_set_op(c.k, c.off, c.k, c.off, "xor")),
    ("set_op.op_number", C, lambda r, c: r.segmented_set_op(c.k, c.off, c.k, c.off, 4)),
    ("set_op.op_bool", C, lambda r, c: r.segmented_set_op(c.k, c.off, c.k, c.off, True)),
    ("set_op.match_without_intersection", C, lambda r, c: r.segmented_set_op(c.k, c.off, c.k, c.off, "union", return_match=True)),
    ("set_op.host", C, lambda r, c: r.segmented_set_op(c.k, c.off, c.k, c.off, "union")),
    ("set_op.host_b", G, lambda r, c: r.segmented_set_op(c.k, c.off, c.host, c.off, "union")),
    ("set_op.keys_2d", G, lambda r, c: r.segmented_set_op(c.k, c.off, c.k2d, c.off, "union")),
    ("set_op.one_offsets", G, lambda r, c: r.segmented_set_op(c.k, None, c.k, c.off, "union")),
    ("set_op.a_offsets_2d", G, lambda r, c: r.segmented_set_op(c.k, c.off2d, c.k, c.off, "union")),
    ("set_op.b_offsets_dtype", G, lambda r, c: r.segmented_set_op(c.k, c.off, c.k, c.off32, "union")),
    ("set_op.b_offsets_host", G, lambda r, c: r.segmented_set_op(c.k, c.off, c.k, c.host_off, "union")),
    ("set_op.offsets_count", G, lambda r, c: r.segmented_set_op(c.k, c.off4, c.k, c.off, "union")),
    ("set_op.one_payload", G, lambda r, c: r.segmented_set_op(c.k, c.off, c.k, c.off, "union", payload_b=c.p)),
    ("set_op.payload_a_shape", G, lambda r, c: r.segmented_set_op(c.k, c.off, c.k, c.off, "union", payload_a=c.p[:5], payload_b=c.p)),
    ("set_op.payload_b_dtype", G, lambda r, c: r.segmented_set_op(c.k, c.off, c.k, c.off, "union", payload_a=c.p, payload_b=c.v)),
    ("set_op.payload_dtypes", G, lambda r, c: r.segmented_set_op(c.k, c.off, c.k, c.off, "union", payload_a=c.pu, payload_b=c.p)),
    ("set_op.too_many", G, lambda r, c: r.segmented_set_op(c.k, None, c.huge, None, "union")),
    ("set_rows.no_tensor", C, lambda r, c: r.intersect_sorted(c.k, [1, 2])),
    ("set_rows.dimensions", C, lambda r, c: r.difference_sorted(c.k, c.k2d)),
    ("set_rows.scalar", C, lambda r, c: r.union_sorted(c.k[0], c.k[0])),
    ("set_rows.payload_shape", C, lambda r, c: r.symmetric_difference_sorted(c.k, c.k, payload_a=c.p, payload_b=c.p[:5])),
    ("set_rows.host", C, lambda r, c: r.intersect_sorted(c.k, c.k)),
    ("set_rows.key_type", C, lambda r, c: r.union_sorted(c.h, c.h)),
    # -- segmented_join, join_sorted, isin_sorted
    ("join.no_tensor", C, lambda r, c: r.segmented_join(c.k, c.off, None, c.off)),
    ("join.key_type", C, lambda r, c: r.segmented_join(c.h, c.off, c.h, c.off)),
    ("join.key_type_and_kind", C, lambda r, c: r.segmented_join(c.h, c.off, c.h, c.off, how="outer")),
    ("join.dtypes", C, lambda r, c: r.segmented_join(c.k, c.off, c.kf, c.off)),
    ("join.dtypes_and_kind", C, lambda r, c: r.segmented_join(c.k, c.off, c.kf, c.off, how="outer")),
    ("join.kind_name", C, lambda r, c: r.segmented_join(c.k, c.off, c.k, c.off, how="outer")),
    ("join.kind_number", C, lambda r, c: r.segmented_join(c.k, c.off, c.k, c.off, how=-1)),
    ("join.host", C, lambda r, c: r.segmented_join(c.k, c.off, c.k, c.off)),
    ("join.host_a", G, lambda r, c: r.segmented_join(c.host, c.off, c.k, c.off)),
    ("join.keys_2d", G, lambda r, c: r.segmented_join(c.k2d, c.off, c.k, c.off)),
    ("join.one_offsets", G, lambda r, c: r.segmented_join(c.k, c.off, c.k, None)),
    ("join.a_offsets_dtype", G, lambda r, c: r.segmented_join(c.k, c.off32, c.k, c.off)),
    ("join.b_offsets_2d", G, lambda r, c: r.segmented_join(c.k, c.off, c.k, c.off2d)),
    ("join.a_offsets_host", G, lambda r, c: r.segmented_join(c.k, c.host_off, c.k, c.off)),
    ("join.offsets_count", G, lambda r, c: r.segmented_join(c.k, c.off, c.k, c.off4)),
    ("join.capacity_negative", G, lambda r, c: r.segmented_join(c.k, c.off, c.k, c.off, capacity=-1)),
    ("join.capacity_float", G, lambda r, c: r.segmented_join(c.k, c.off, c.k, c.off, capacity=4.0)),
    ("join.capacity_bool", G, lambda r, c: r.segmented_join(c.k, c.off, c.k, c.off, capacity=True)),
    ("join.capacity_large", G, lambda r, c: r.segmented_join(c.k, c.off, c.k, c.off, capacity=(1 << 34) + 1)),
    ("join.too_many_a", G, lambda r, c: r.segmented_join(c.huge, None, c.k, None)),
    ("join.too_many_b", G, lambda r, c: r.segmented_join(c.k, None, c.huge, None, capacity=4)),
    ("join_rows.no_tensor", C, lambda r, c: r.join_sorted(c.k, 3)),
    ("join_rows.dimensions", C, lambda r, c: r.join_sorted(c.k2d, c.k)),
    ("join_rows.host", C, lambda r, c: r.join_sorted(c.k, c.k)),
    ("join_rows.kind", C, lambda r, c: r.join_sorted(c.k, c.k, how="outer")),
    ("isin_sorted.no_tensor", C, lambda r, c: r.isin_sorted([1], c.k)),
    ("isin_sorted.host", C, lambda r, c: r.isin_sorted(c.k2d, c.k2d)),
    ("isin_sorted.dtypes", C, lambda r, c: r.isin_sorted(c.k, c.k64)),
]
IDS = [row[0] for row in ROWS]
assert len(set(IDS)) == len(IDS)


def refusal(rsx, ctx, call):
    """[exception class name, message] of a bad call; a call that passes is recorded as such and matches no golden entry"""
    try:
        call(rsx, ctx)
    except Exception as e:          # noqa: BLE001  (the class is what is pinned)
        return [type(e).__name__, str(e)]
    return ["no exception", ""]


@pytest.fixture(scope="module")
def pinned():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def host_ctx():
    return Ctx(pytest.importorskip("torch"), "cpu")


@pytest.fixture(scope="module")
def device_ctx():
    return Ctx(pytest.importorskip("torch"), "cuda")


def test_argument_module_tables_match_the_binding(rsx):
    """the dtype tables live in the argument module, which knows nothing of the binding: their numbers are the binding's constants"""
    assert rsx._KEY_DTYPES is rsx._args.KEY_DTYPES and rsx._VALUE_KINDS is rsx._args.VALUE_KINDS
    assert rsx._KEY_DTYPES == {"uint32": (4, rsx.KEY_UNSIGNED), "int32": (4, rsx.KEY_SIGNED), "uint64": (8, rsx.KEY_UNSIGNED),
                               "int64": (8, rsx.KEY_SIGNED), "float32": (4, rsx.KEY_FLOAT), "float64": (8, rsx.KEY_FLOAT)}
    assert rsx._VALUE_KINDS == {"int32": rsx.VALUE_INT32, "int64": rsx.VALUE_INT64, "float32": rsx.VALUE_FLOAT32, "float64": rsx.VALUE_FLOAT64}
    assert rsx._aligned_copy is rsx._args.aligned_copy and rsx._args.MAX_ELEMENTS == 1 << 31


def test_every_row_is_pinned(pinned):
    assert sorted(pinned) == sorted(IDS)
    assert all(cls != "no exception" for cls, _ in pinned.values())


@pytest.mark.parametrize("rid,call", [(i, f) for i, g, f in ROWS if not g], ids=[i for i, g, _ in ROWS if not g])
def test_host_refusal(rsx, pinned, host_ctx, rid, call):
    assert refusal(rsx, host_ctx, call) == pinned[rid]


@pytest.mark.gpu
@pytest.mark.parametrize("rid,call", [(i, f) for i, g, f in ROWS if g], ids=[i for i, g, _ in ROWS if g])
def test_device_refusal(rsx, pinned, device_ctx, rid, call):
    assert refusal(rsx, device_ctx, call) == pinned[rid]


if __name__ == "__main__":
    import torch
    from _loader import load_package
    rsx_ = load_package()
    host, device = Ctx(torch, "cpu"), (Ctx(torch, "cuda") if torch.cuda.is_available() else None)
    found = {i: refusal(rsx_, device if g else host, f) for i, g, f in ROWS if device is not None or not g}
    with open(sys.argv[1], "w") as out:
        json.dump(found, out, indent=1, sort_keys=True)
        out.write("\n")
    print(f"{len(found)} of {len(ROWS)} rows recorded")
