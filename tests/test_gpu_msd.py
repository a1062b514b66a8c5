"""The exchange step of the sharded sort on the top B <= 8 key bits (rsx_msd_count / _scatter / _plan / _push) against numpy
and against the host planner (radix-sort_amd/host/ShardPlanner, the ONE implementation the Python and C++ drivers share):
counts, the wave-major staging order, the device-side plan, and the pushed receive buffers of all ranks of a world emulated on
the one GPU (every "rank" is an engine of this process; the receive buffers are plain device tensors)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _unsigned(keys):
    bits = keys.dtype.itemsize * 8
    u = keys.view(np.uint32 if bits == 32 else np.uint64)
    if keys.dtype.kind == "i":
        u = u ^ u.dtype.type(1 << (bits - 1))
    return u, bits


def _position(top_byte, bits, world):
    """wave-major position of a fine bucket (the key's top byte): [wave][rank][low 8 - bits bits]"""
    sub_shift = 8 - bits
    c, sub = top_byte >> sub_shift, top_byte & ((1 << sub_shift) - 1)
    k = (1 << bits) // world
    return (((c % k) * world + c // k) << sub_shift) | sub


@pytest.mark.parametrize("dt,bits,world,payload", [("uint32", 4, 8, False), ("uint32", 6, 8, False), ("int32", 8, 8, True), ("uint64", 5, 4, True), ("int64", 8, 16, False),
                                                    ("uint32", 3, 8, True), ("uint64", 1, 2, False), ("uint32", 8, 1, False), ("int64", 6, 2, True)])
def test_count_and_wave_major_scatter(rsx, oracle, dt, bits, world, payload):
    import torch
    n = 300007
    keys = oracle.dataset("SeededUniform", dt, n, seed=bits * 17 + world)
    keys[::7] = keys[3]
    u, kb = _unsigned(keys)
    top = (u >> u.dtype.type(kb - 8)).astype(np.int64)
    coarse = top >> (8 - bits)
    signed = {"uint32": np.int32, "uint64": np.int64}.get(np.dtype(dt).name)
    tk = torch.from_numpy(keys.view(signed) if signed else keys).cuda()
    pay = torch.arange(n, dtype=torch.int32, device="cuda") if payload else None
    staging = torch.empty_like(tk)
    spay = torch.empty_like(pay) if payload else None
    row = torch.full((259,), -1, dtype=torch.int64, device="cuda")
    with rsx.Engine(dt, n, payload=payload) as e:
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        for _ in range(2):                                   # twice: the tables are reused
            e.msd_count(tk.data_ptr(), n, bits, world, row.data_ptr())
            e.msd_scatter(tk.data_ptr(), n, staging.data_ptr(), pay.data_ptr() if payload else None, spay.data_ptr() if payload else None)
            torch.cuda.synchronize()
            want = np.bincount(coarse, minlength=256)
            assert row[:256].cpu().tolist() == [int(v) for v in want] and row[256:].cpu().tolist() == [-1, -1, -1]
            order = np.argsort(_position(top, bits, world), kind="stable")
            assert np.array_equal(staging.cpu().numpy().view(keys.dtype), keys[order])
            if payload:
                assert np.array_equal(spay.cpu().numpy().view(np.uint32), order.astype(np.uint32))
        with pytest.raises(rsx.RadixSortError):              # the count was consumed
            e.msd_scatter(tk.data_ptr(), n, staging.data_ptr(), pay.data_ptr() if payload else None, spay.data_ptr() if payload else None)
        for bad_bits, bad_world in ((0, 1), (9, 8), (4, 3), (2, 8), (4, 32)):
            with pytest.raises(rsx.RadixSortError):
                e.msd_count(tk.data_ptr(), n, bad_bits, bad_world, row.data_ptr())
        e.msd_count(tk.data_ptr(), 0, bits, world, row.data_ptr())
        torch.cuda.synchronize()
        assert row[:256].cpu().tolist() == [0] * 256
        # the engine still sorts (the 8-bit tables were borrowed, not broken)
        e.sort_from(tk.data_ptr(), n, pay.data_ptr() if payload else None)
        assert np.array_equal(e.download(), np.sort(keys))


@pytest.mark.parametrize("dt,bits,world,payload,grouping", [("uint32", 6, 8, False, 1), ("uint32", 4, 8, True, 0), ("int64", 8, 4, True, 1), ("uint64", 5, 2, False, 1), ("int32", 8, 16, False, 0),
                                                             ("uint32", 6, 8, True, 0)])
def test_device_plan_and_push_fill_every_receive_buffer(rsx, oracle, dt, bits, world, payload, grouping):
    """A whole world on the one GPU: every rank counts and scatters its shard, the [rank][bucket] table is assembled as the all_gather
    would, every rank plans on the device and pushes wave by wave into the receive buffers of all ranks.  Afterwards rank d's buffer holds,
    wave by wave (16-byte aligned), the keys of bucket d * k + w of rank 0, 1, ... in order — checked against numpy — and the plan the
    host reads back equals the host planner's for the same table."""
    import torch
    from radix_sort_amd import planner
    n = 120011
    full = oracle.dataset("SeededUniform", dt, n * world, seed=bits + 100 * world)
    full[::5] = full[2]
    u_all, kb = _unsigned(full)
    signed = {"uint32": np.int32, "uint64": np.int64}.get(np.dtype(dt).name)
    tdt = torch.int32 if kb == 32 else torch.int64
    cap = 4 * n + 4 * 256          # the tie value (a fifth of all keys) lands on one rank
    waves = (1 << bits) // world
    stride = 259
    table = torch.zeros(world * stride, dtype=torch.int64, device="cuda")
    engines = [rsx.Engine(dt, n, payload=payload) for _ in range(world)]
    try:
        shards, stagings, spays, recvs, rpays = [], [], [], [], []
        for r, e in enumerate(engines):
            e.set_stream(torch.cuda.current_stream().cuda_stream)
            shard = full[r * n:(r + 1) * n]
            tk = torch.from_numpy((shard.view(signed) if signed else shard).copy()).cuda()
            pay = torch.arange(r * n, (r + 1) * n, dtype=torch.int32, device="cuda") if payload else None
            shards.append((tk, pay))
            stagings.append(torch.empty_like(tk))
            spays.append(torch.empty_like(pay) if payload else None)
            recvs.append(torch.full((cap,), -7, dtype=tdt, device="cuda"))
            rpays.append(torch.full((cap,), -7, dtype=torch.int32, device="cuda") if payload else None)
            e.msd_count(tk.data_ptr(), n, bits, world, table[r * stride:].data_ptr())
            e.msd_scatter(tk.data_ptr(), n, stagings[r].data_ptr(), pay.data_ptr() if payload else None, spays[r].data_ptr() if payload else None)
            table[r * stride + 256] = cap          # receive capacity
            table[r * stride + 257] = cap          # output capacity
        peer_k = torch.tensor([t.data_ptr() for t in recvs], dtype=torch.int64, device="cuda")
        peer_p = torch.tensor([t.data_ptr() for t in rpays], dtype=torch.int64, device="cuda") if payload else None
        torch.cuda.synchronize()
        host_table = table.cpu().view(world, stride).numpy()
        side = torch.cuda.Stream()
        plans = []
        for r, e in enumerate(engines):
            side.wait_stream(torch.cuda.current_stream())
            e.msd_plan(table.data_ptr(), stride, 256, r, side.cuda_stream if r % 2 else 0, grouping)      # odd ranks plan on a side stream
            plans.append(e.msd_plan_wait(waves, world))
            for w in range(waves):
                e.msd_push(w, stagings[r].data_ptr(), peer_k.data_ptr(), spays[r].data_ptr() if payload else None, peer_p.data_ptr() if payload else None, parts=(r % 3) * 7)
        torch.cuda.synchronize()
        counts = [[int(v) for v in host_table[r, :1 << bits]] for r in range(world)]
        start, offset, loads = planner.wave_layout(counts, world, 1 << bits, 4, grouping)
        top_all = (u_all >> u_all.dtype.type(kb - bits)).astype(np.int64)
        for d in range(world):
            ws, wc, ld, verdict = plans[d]
            assert verdict == 0 and ld == loads and ws == start[d]
            got = recvs[d].cpu().numpy().view(full.dtype)
            gotp = rpays[d].cpu().numpy().view(np.uint32) if payload else None
            used = np.zeros(cap, dtype=bool)
            for w in range(waves):
                b = d * waves + w
                assert wc[w] == sum(counts[s][b] for s in range(world))
                for s in range(world):
                    idx = np.flatnonzero(top_all[s * n:(s + 1) * n] == b) + s * n
                    # inside a segment the keys are grouped (stably) by the remaining bits of the top byte
                    sub = (u_all[idx] >> u_all.dtype.type(kb - 8)).astype(np.int64)
                    idx = idx[np.argsort(sub, kind="stable")]
                    at = offset[d][w][s]
                    assert np.array_equal(got[at:at + idx.size], full[idx]), (d, w, s)
                    if payload:
                        assert np.array_equal(gotp[at:at + idx.size], idx.astype(np.uint32)), (d, w, s)
                    used[at:at + idx.size] = True
            raw = recvs[d].cpu().numpy()
            assert (raw[~used] == -7).all()                 # nothing outside the segments
    finally:
        for e in engines:
            e.close()


def test_plan_verdict_when_a_rank_is_too_small(rsx, oracle):
    """One rank's receive buffer is too small: every rank's plan carries the same verdict and no push writes anything."""
    import torch
    world, bits, n = 4, 4, 50000
    full = oracle.dataset("SeededUniform", "uint32", n * world, seed=3)
    stride = 259
    table = torch.zeros(world * stride, dtype=torch.int64, device="cuda")
    engines = [rsx.Engine("uint32", n) for _ in range(world)]
    try:
        stagings, recvs = [], []
        for r, e in enumerate(engines):
            e.set_stream(torch.cuda.current_stream().cuda_stream)
            tk = torch.from_numpy(full[r * n:(r + 1) * n].view(np.int32).copy()).cuda()
            stagings.append(torch.empty_like(tk))
            recvs.append(torch.full((2 * n,), -7, dtype=torch.int32, device="cuda"))
            e.msd_count(tk.data_ptr(), n, bits, world, table[r * stride:].data_ptr())
            e.msd_scatter(tk.data_ptr(), n, stagings[r].data_ptr())
            table[r * stride + 256] = 2 * n if r != 2 else n // 2
            table[r * stride + 257] = 2 * n
        peer_k = torch.tensor([t.data_ptr() for t in recvs], dtype=torch.int64, device="cuda")
        for r, e in enumerate(engines):
            e.msd_plan(table.data_ptr(), stride, 256, r)
            assert e.msd_plan_wait(4, world)[3] == 1 << 2
            for w in range(4):
                e.msd_push(w, stagings[r].data_ptr(), peer_k.data_ptr())
        torch.cuda.synchronize()
        for t in recvs:
            assert (t == -7).all()
        with pytest.raises(rsx.RadixSortError):
            engines[0].msd_push(4, stagings[0].data_ptr(), peer_k.data_ptr())
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("dt,bits,world,payload,grouping,sizes", [
    ("uint32", 6, 8, False, 1, [0, 1, 2, 3, 6000, 30011, 4096, 777]),
    ("int64", 8, 4, True, 0, [3, 0, 20000, 1]),
    ("int32", 5, 4, True, 1, [2, 4097, 0, 12345]),
    ("uint64", 4, 2, False, 0, [9999, 1]),
    ("uint32", 8, 16, True, 1, [0, 3, 1, 2, 0, 5000, 0, 0, 64, 0, 0, 7, 4095, 0, 0, 1]),
])
def test_device_plan_with_uneven_shards_and_exact_capacities(rsx, oracle, dt, bits, world, payload, grouping, sizes):
    """The exchange kernels with shards of different sizes (0, 1, 2, 3 keys, and a shard whose keys all fall into ONE fine bucket) and every
    receive buffer exactly as large as the extent of its wave layout (host planner's wave_extents), every output capacity exactly its load:
    the device plan says go, loads / wave starts / wave counts equal the host planner's, every key lands in its slot up to the last one and
    the sentinel slots behind the extent stay untouched.  Then one rank's capacity is one slot short: every rank's plan carries verdict
    1 << r and no push writes a byte anywhere."""
    import torch
    from radix_sort_amd import planner
    stride, sentinel = 259, 8
    total = sum(sizes)
    full = oracle.dataset("SeededUniform", dt, total, seed=bits * 7 + world)
    u_all, kb = _unsigned(full)
    bounds = np.cumsum([0] + sizes)
    one = max(range(world), key=lambda r: (sizes[r] >= 4, r == world // 2))        # this shard's keys share one top byte
    lo, hi = int(bounds[one]), int(bounds[one + 1])
    raw = full.view(u_all.dtype)
    raw[lo:hi] = (raw[lo:hi] & u_all.dtype.type((1 << (kb - 8)) - 1)) | u_all.dtype.type(0x5A << (kb - 8))
    u_all, _ = _unsigned(full)
    signed = {"uint32": np.int32, "uint64": np.int64}.get(np.dtype(dt).name)
    tdt = torch.int32 if kb == 32 else torch.int64
    waves = (1 << bits) // world
    top_all = (u_all >> u_all.dtype.type(kb - bits)).astype(np.int64)
    counts = [[int(v) for v in np.bincount(top_all[bounds[r]:bounds[r + 1]], minlength=1 << bits)] for r in range(world)]
    assert sum(c > 0 for c in counts[one]) == (1 if sizes[one] else 0)
    start, offset, loads = planner.wave_layout(counts, world, 1 << bits, 4, grouping)
    extents = planner.wave_extents(counts, world, 1 << bits, 4, grouping)
    table = torch.zeros(world * stride, dtype=torch.int64, device="cuda")
    engines = [rsx.Engine(dt, max(n, 16), payload=payload) for n in sizes]
    try:
        stagings, spays, recvs, rpays = [], [], [], []
        for r, e in enumerate(engines):
            e.set_stream(torch.cuda.current_stream().cuda_stream)
            shard = full[bounds[r]:bounds[r + 1]]
            tk = torch.from_numpy((shard.view(signed) if signed else shard).copy()).cuda()
            pay = torch.arange(int(bounds[r]), int(bounds[r + 1]), dtype=torch.int32, device="cuda") if payload else None
            stagings.append(torch.empty_like(tk))
            spays.append(torch.empty_like(pay) if payload else None)
            recvs.append(torch.full((extents[r] + sentinel,), -7, dtype=tdt, device="cuda"))
            rpays.append(torch.full((extents[r] + sentinel,), -7, dtype=torch.int32, device="cuda") if payload else None)
            e.msd_count(tk.data_ptr(), sizes[r], bits, world, table[r * stride:].data_ptr())
            e.msd_scatter(tk.data_ptr(), sizes[r], stagings[r].data_ptr(), pay.data_ptr() if payload else None, spays[r].data_ptr() if payload else None)
        torch.cuda.synchronize()
        assert [[int(v) for v in row[:1 << bits]] for row in table.cpu().view(world, stride).tolist()] == counts
        peer_k = torch.tensor([t.data_ptr() for t in recvs], dtype=torch.int64, device="cuda")
        peer_p = torch.tensor([t.data_ptr() for t in rpays], dtype=torch.int64, device="cuda") if payload else None

        def step(caps):
            for r in range(world):
                table[r * stride + 256], table[r * stride + 257] = caps[r]
            plans = []
            for r, e in enumerate(engines):
                e.msd_plan(table.data_ptr(), stride, 256, r, 0, grouping)
                plans.append(e.msd_plan_wait(waves, world))
                for w in range(waves):
                    e.msd_push(w, stagings[r].data_ptr(), peer_k.data_ptr(), spays[r].data_ptr() if payload else None, peer_p.data_ptr() if payload else None)
            torch.cuda.synchronize()
            return plans

        plans = step(list(zip(extents, loads)))
        for d in range(world):
            ws, wc, ld, verdict = plans[d]
            assert verdict == 0 and ld == loads and ws == start[d]
            assert wc == [sum(counts[s][d * waves + w] for s in range(world)) for w in range(waves)]
            got = recvs[d].cpu().numpy().view(full.dtype)
            gotp = rpays[d].cpu().numpy().view(np.uint32) if payload else None
            used = np.zeros(extents[d] + sentinel, dtype=bool)
            for w in range(waves):
                for s in range(world):
                    idx = np.flatnonzero(top_all[bounds[s]:bounds[s + 1]] == d * waves + w) + bounds[s]
                    sub = (u_all[idx] >> u_all.dtype.type(kb - 8)).astype(np.int64)
                    idx = idx[np.argsort(sub, kind="stable")]
                    at = offset[d][w][s]
                    assert at + idx.size <= extents[d]
                    assert np.array_equal(got[at:at + idx.size], full[idx]), (d, w, s)
                    if payload:
                        assert np.array_equal(gotp[at:at + idx.size], idx.astype(np.uint32)), (d, w, s)
                    used[at:at + idx.size] = True
            assert used.sum() == loads[d]
            assert (recvs[d].cpu().numpy()[~used] == -7).all()                              # gaps and the sentinel behind the extent untouched
            if payload:
                assert (rpays[d].cpu().numpy()[~used] == -7).all()
        # one slot short on one rank (the one with the largest extent): the same verdict everywhere, nothing written
        short = max(range(world), key=lambda r: extents[r])
        for t in recvs + [p for p in rpays if p is not None]:
            t.fill_(-7)
        plans = step([(e - (r == short), l) for r, (e, l) in enumerate(zip(extents, loads))])
        assert all(p[3] == 1 << short for p in plans), [p[3] for p in plans]
        for t in recvs + [p for p in rpays if p is not None]:
            assert (t == -7).all()
    finally:
        for e in engines:
            e.close()
