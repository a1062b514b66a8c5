"""Host referee of the unique tests (rsx_segmented_unique), per segment, on the unsigned image of the key under the engine's order map (enc of
tests/test_gpu_float_keys.py, complemented for descending engines: the map _topk_ref / _select_ref use), in two forms.

unique_oracle   the numpy form: np.unique(image, return_index, return_inverse, return_counts) per segment in sorted mode (numpy's
                return_index is the FIRST occurrence), a != on neighbours in consecutive mode.
slow_unique     the same answer from a dict / a loop over the elements, to check the fast form against.
Both return a dict: keys (packed distinct keys, unsigned words of the INPUT bits), run_offsets (S + 1 uint64), counts, first (uint32,
packed like keys), inverse (uint32, n entries) and written (bool, n entries: the positions of inverse the call writes, i.e. [off[0], off[S])).
off None = one segment [0, n).
"""
import numpy as np

from test_gpu_float_keys import UINT, enc


def _image(x, descending):
    e = enc(x)
    return ~e if descending else e


def _offsets(off, n):
    return np.array([0, n], dtype=np.int64) if off is None else np.asarray(off, dtype=np.int64)


def _pack(x, off, parts):
    n = x.size
    u = UINT[x.dtype]
    nseg = len(off) - 1
    keys, counts, first = [], [], []
    inverse = np.zeros(n, dtype=np.uint32)
    written = np.zeros(n, dtype=bool)
    uoff = np.zeros(nseg + 1, dtype=np.uint64)
    for s, (k, c, f, inv) in enumerate(parts):
        a, b = int(off[s]), int(off[s + 1])
        keys.append(k)
        counts.append(c)
        first.append(f)
        inverse[a:b] = inv
        written[a:b] = True
        uoff[s + 1] = uoff[s] + np.uint64(len(k))
    cat = lambda parts_, dt: np.concatenate(parts_).astype(dt) if parts_ else np.zeros(0, dtype=dt)
    return {"keys": cat(keys, u), "run_offsets": uoff, "counts": cat(counts, np.uint32), "first": cat(first, np.uint32), "inverse": inverse,
            "written": written}


def unique_oracle(x: np.ndarray, off=None, descending: bool = False, consecutive: bool = False):
    n = x.size
    off = _offsets(off, n)
    xu = x.view(UINT[x.dtype])
    img = _image(x, descending)
    parts = []
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        assert 0 <= a <= b <= n, "the referee takes valid offsets only"
        seg = img[a:b]
        if consecutive:
            head = np.ones(b - a, dtype=bool)
            head[1:] = seg[1:] != seg[:-1]
            f = np.flatnonzero(head)
            c = np.diff(np.append(f, b - a))
            inv = np.cumsum(head) - 1
        else:
            _, f, inv, c = np.unique(seg, return_index=True, return_inverse=True, return_counts=True)
            inv = inv.reshape(-1)
        parts.append((xu[a:b][f], c, f, inv))
    return _pack(x, off, parts)


def slow_unique(x: np.ndarray, off=None, descending: bool = False, consecutive: bool = False):
    n = x.size
    off = _offsets(off, n)
    xu = x.view(UINT[x.dtype])
    img = _image(x, descending).tolist()
    parts = []
    for s in range(len(off) - 1):
        a, b = int(off[s]), int(off[s + 1])
        runs = []                                   # [image, first position, count]
        inv = []
        if consecutive:
            for i in range(a, b):
                if i == a or img[i] != img[i - 1]:
                    runs.append([img[i], i - a, 0])
                runs[-1][2] += 1
                inv.append(len(runs) - 1)
        else:
            seen = {}
            for i in range(a, b):
                r = seen.get(img[i])
                if r is None:
                    r = seen[img[i]] = [img[i], i - a, 0]
                r[2] += 1
            runs = sorted(seen.values())
            rank = {r[0]: j for j, r in enumerate(runs)}
            inv = [rank[img[i]] for i in range(a, b)]
        f = np.array([r[1] for r in runs], dtype=np.int64)
        parts.append((xu[a:b][f] if len(runs) else xu[:0], np.array([r[2] for r in runs], dtype=np.int64), f, np.array(inv, dtype=np.int64)))
    return _pack(x, off, parts)


FIELDS = ("keys", "run_offsets", "counts", "first", "inverse", "written")


def same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in FIELDS)
