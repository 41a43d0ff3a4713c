"""The bucket table of a saved image, restated for the tests: the hash, the home bucket and the walk of
kaamer_layout.h, the key encoding in its closed form, and the arena's lists -- scalar forms (one key at a time, as
tests/test_arena_order.py reads them) and vectorised numpy forms (a whole batch of windows at once, with the number
of buckets every lookup walks: what the probe kernel's n_probe counter must add up to).

Test infrastructure only.  Nothing here calls the library except to obtain the saved image bytes."""
import os

import numpy as np

EMPTY = 0xFFFFFFFF
INLINE = 0x80000000
KMER_SIZE = 7


def _mix32(h):   # kaamer_layout.h kh_mix32
    h ^= h >> 16
    h = (h * 0x85ebca6b) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def _shard_of(key, n_shards):
    return (_mix32(key) * n_shards) >> 32


def _home(key, n_shards, n_buckets):
    rest = (_mix32(key) * n_shards) & 0xFFFFFFFF
    return (rest * n_buckets) >> 32


def _image_bytes(img, tmp_path, name="a.kgi"):
    p = os.path.join(str(tmp_path), name)
    img.save(p)
    with open(p, "rb") as f:
        b = f.read()
    os.unlink(p)
    return b


# ---- vectorised forms ---------------------------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def mix32_v(keys):
    """kh_mix32 of a uint32 array -> uint64 array of 32-bit values"""
    h = np.asarray(keys).astype(np.uint64)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85ebca6b)) & _M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xc2b2ae35)) & _M32
    h ^= h >> np.uint64(16)
    return h


def shard_of_v(keys, n_shards):
    return ((mix32_v(keys) * np.uint64(n_shards)) >> np.uint64(32)).astype(np.int64)


def home_v(keys, n_shards, n_buckets):
    rest = (mix32_v(keys) * np.uint64(n_shards)) & _M32
    return ((rest * np.uint64(n_buckets)) >> np.uint64(32)).astype(np.int64)


def _code_lut():
    """kh_residue_code: index in "ACDEFGHIKLMNPQRSTUVWY", 30 for '.', 31 for every other byte"""
    lut = np.full(256, 31, dtype=np.uint32)
    for i, c in enumerate(b"ACDEFGHIKLMNPQRSTUVWY"):
        lut[c] = i
    lut[ord(".")] = 30
    return lut


_LUT = _code_lut()


def _pair(a, b):
    """kh_pair: 22 + 21 a + b for two letters of the alphabet, a when the second one is '.', else 0"""
    both = np.uint32(22) + np.uint32(21) * a + b
    r = np.where(b < 21, both, np.where(b == 30, a, np.uint32(0)))
    return np.where(a < 21, r, np.uint32(0)).astype(np.uint32)


def encode_windows(buf, starts):
    """keys (uint32) of the 7-residue windows of the byte buffer `buf` that begin at `starts`"""
    buf = np.frombuffer(bytes(buf), dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else np.asarray(buf, dtype=np.uint8)
    starts = np.asarray(starts, dtype=np.int64)
    if len(starts) == 0:
        return np.zeros(0, np.uint32)
    c = _LUT[buf[starts[:, None] + np.arange(KMER_SIZE)[None, :]]]
    last = np.where(c[:, 6] < 21, c[:, 6], np.uint32(0)).astype(np.uint32)
    return ((_pair(c[:, 0], c[:, 1]) << np.uint32(23)) | (_pair(c[:, 2], c[:, 3]) << np.uint32(14)) |
            (_pair(c[:, 4], c[:, 5]) << np.uint32(5)) | last).astype(np.uint32)


def window_starts(offs, sizes):
    """start positions (in the packed buffer) of the first sizes[i] windows of every sequence i, in order"""
    offs = np.asarray(offs).astype(np.int64)
    sizes = np.maximum(np.asarray(sizes, dtype=np.int64), 0)
    total = int(sizes.sum())
    first = np.zeros(len(sizes), dtype=np.int64)
    first[1:] = np.cumsum(sizes[:-1])
    return np.repeat(offs[:len(sizes)] - first, sizes) + np.arange(total, dtype=np.int64)


def db_window_keys(packed):
    """keys of every window a builder emits for the packed proteins (len - 6 per protein of 7 residues or more)"""
    buf, offs = packed
    lens = np.diff(np.asarray(offs).astype(np.int64))
    return encode_windows(buf, window_starts(offs, lens - (KMER_SIZE - 1)))


class _Table:
    """buckets and arena of a saved image, and the lookup of kaamer_layout.h"""

    def __init__(self, raw, st):
        w = np.frombuffer(raw, dtype=np.uint32)
        self.nb = st["n_buckets"]
        self.n_shards = st["n_shards"]
        self.shard = st["shard"]
        self.slots = w[1024:1024 + self.nb * 16].reshape(self.nb, 8, 2)
        self.arena = w[1024 + self.nb * 16:]
        assert len(self.arena) == st["arena_words"]

    def val(self, key):
        b = _home(key, self.n_shards, self.nb)
        for _ in range(self.nb):
            ks = self.slots[b, :, 0]
            at = np.flatnonzero(ks == key)
            if len(at):
                return int(self.slots[b, at[0], 1])
            if (ks == EMPTY).any():
                return None
            b = 0 if b + 1 == self.nb else b + 1
        return None

    def units(self, off):
        return (1 + int(self.arena[off * 4]) + 3) // 4

    def ids(self, val):
        if val & INLINE:
            return [val & ~INLINE]
        c = int(self.arena[val * 4])
        return self.arena[val * 4 + 1:val * 4 + 1 + c].tolist()

    def walk(self, keys):
        """The lookup of every key at once -> (val, n_buckets_walked, wrapped).

        A lookup starts at the key's home bucket; it stops on a slot that holds the key (val = the slot's value), else
        on a bucket with an empty slot (val = 0: the key is absent), else goes to the next bucket modulo n_buckets, and
        gives up after n_buckets buckets.  n_buckets_walked counts the buckets it read; wrapped says that it went from
        the last bucket on to bucket 0.  A shard's table skips the keys another shard owns: val 0, no bucket read."""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        n = len(keys)
        val = np.zeros(n, dtype=np.uint32)
        walked = np.zeros(n, dtype=np.int64)
        wrapped = np.zeros(n, dtype=bool)
        if n == 0:
            return val, walked, wrapped
        live = np.arange(n)
        if self.n_shards > 1:
            live = np.flatnonzero(shard_of_v(keys, self.n_shards) == self.shard)
        b = home_v(keys[live], self.n_shards, self.nb)
        for step in range(self.nb):
            if len(live) == 0:
                break
            walked[live] += 1
            ks = self.slots[b, :, 0]
            hit = ks == keys[live][:, None]
            found = hit.any(axis=1)
            val[live[found]] = self.slots[b[found], hit[found].argmax(axis=1), 1]
            go = ~found & ~(ks == EMPTY).any(axis=1)
            if step + 1 == self.nb:
                break
            live, b = live[go], b[go] + 1
            last = b == self.nb
            wrapped[live[last]] = True
            b[last] = 0
        return val, walked, wrapped

    def ids_csr(self, vals):
        """the protein ids behind slot values (none of them 0) -> (offsets int64[n + 1], ids uint32)"""
        vals = np.asarray(vals, dtype=np.uint32)
        inline = (vals & np.uint32(INLINE)) != 0
        at = np.where(inline, 0, vals).astype(np.int64) * 4
        cnt = np.where(inline, 1, self.arena[at]).astype(np.int64)
        off = np.zeros(len(vals) + 1, dtype=np.int64)
        np.cumsum(cnt, out=off[1:])
        src = np.repeat(at + 1 - off[:-1], cnt) + np.arange(int(off[-1]), dtype=np.int64)
        ids = self.arena[np.where(np.repeat(inline, cnt), 0, src)]
        ids[off[:-1][inline]] = vals[inline] & np.uint32(~INLINE & 0xFFFFFFFF)
        return off, ids


def table_of(img, tmp_path, name="t.kgi"):
    return _Table(_image_bytes(img, tmp_path, name), img.stats())
