"""tests/blockfmt.py with bitmaps (arrays = 4), without a GPU: a random round trip at W = 3 through the numpy functions
alone, and the section offsets against the library's own layout calls."""
import ctypes as C

import numpy as np
import pytest

import blockfmt as bf

W = 3


def _layout(klib, rank, nq, entries, pos_words, fit=None):
    from kaamer_amd import abi
    cap = abi.ExchangeLayout()
    abi.check(klib.kaamer_exchange_layout_init_positions(W, rank, nq, entries, pos_words, C.byref(cap)))
    if fit is None:
        return cap
    L = abi.ExchangeLayout()
    abi.check(klib.kaamer_exchange_layout_fit_positions(C.byref(cap), *fit, C.byref(L)))
    return L


def _partial_lists(rng, nq, size, r):
    """rank r's partial lists: ids r, r + W, ... would make the ranks' hit sets disjoint, so every rank draws from the same
    ids; bit b of a bitmap belongs to rank b mod W (every k-mer key has one owner: the shards' bitmaps are disjoint)"""
    cnt = rng.integers(0, 6, nq)
    cnt[size < W] = 0                                       # (every rank needs a bit of its own in every bitmap)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    pid, km, fp, pos_off, bits = [], [], [], [], []
    for q in range(nq):
        w = bf.words_of(size[q])
        for p in rng.choice(40, int(cnt[q]), replace=False):
            mine = [b for b in range(int(size[q])) if b % W == r and rng.random() < 0.5] or [r]
            words = [0] * w
            for b in mine:
                words[b >> 6] |= 1 << (b & 63)
            pid.append(int(p)); km.append(len(mine)); fp.append(min(mine))
            pos_off.append(len(bits)); bits += words
    return (off, cnt, np.array(pid, np.uint32), np.array(km, np.uint32), np.array(fp, np.uint32),
            np.array(pos_off, np.int64), np.array(bits, np.uint64))


def test_layout_sections_match_the_library(klib):
    from kaamer_amd import sharded
    for rank, nq, entries, pos_words in ((0, 17, 100, 64), (2, 1000, 5000, 12345), (1, 1, 1, 1)):
        cap = _layout(klib, rank, nq, entries, pos_words)
        fit = _layout(klib, rank, nq, entries, pos_words, fit=(max(1, nq // 3), max(1, entries // 7), max(1, pos_words // 5)))
        for L, pw in ((cap, pos_words), (fit, max(2, max(1, pos_words // 5)))):
            assert L.arrays == 4 and bf.has_bitmaps(L)
            assert bf.ent_base(L) == bf.X_HDR + 2 * L.q_cap
            assert bf.ent_base(L) + 3 * L.e_cap <= bf.bits_off(L) <= bf.ent_base(L) + 3 * L.e_cap + 1 and bf.bits_off(L) % 2 == 0
            assert L.block_words == (bf.bits_off(L) + 2 * pw + 3) & ~3
            assert pw <= bf.p_cap(L) <= pw + 2 and bf.p_cap(L) == sharded.pos_words_of(L)
            assert bf.bits_off(L) + 2 * bf.p_cap(L) <= L.block_words
        assert fit.block_words <= cap.block_words and fit.q_cap <= cap.q_cap and fit.e_cap <= cap.e_cap


@pytest.mark.parametrize("fitted", [False, True], ids=["capacity", "fitted"])
def test_round_trip_with_bitmaps_world3(klib, fitted):
    rng = np.random.default_rng(21)
    nq = 41
    size = rng.integers(-6, 150, nq).astype(np.int32)      # (an empty protein query has SizeInKmer -6; 150: three words)
    parts = [_partial_lists(rng, nq, size, r) for r in range(W)]
    fit = (nq, 5 * nq, 15 * nq) if fitted else None
    layouts = [_layout(klib, r, 64, 400, 1500, fit=fit) for r in range(W)]
    bw = int(layouts[0].block_words)
    sends = []
    for r, (off, cnt, pid, km, fp, pos_off, bits) in enumerate(parts):
        s = bf.pack_blocks(layouts[r], nq, off, cnt, pid, km, fp, True, size=size, pos_off=pos_off, pos_bits=bits)
        sends.append(s)
        m = bf.defined_words(layouts[r], s, True)
        assert not s[~m].any()                             # what the format does not define stays as it was
        for d in range(W):
            h = s[d * bw:d * bw + bf.X_HDR]
            owned = list(range(d, nq, W))
            assert h[bf.X_STATUS] == bf.XS_FIRST_POS | bf.XS_BITMAPS and h[bf.X_NQ] == nq and h[bf.X_OWNED] == len(owned)
            assert h[bf.X_ENTRIES] == h[bf.X_NEED] == int(cnt[owned].sum())
            assert h[bf.X_BITS_NEED] == sum(int(cnt[q]) * bf.words_of(size[q]) for q in owned)
            assert h[bf.X_NEED_MAX] == max(int(cnt[list(range(x, nq, W))].sum()) for x in range(W))
            assert h[bf.X_BITS_NEED_MAX] == max(int(s[x * bw + bf.X_BITS_NEED]) for x in range(W))
            assert s[d * bw + bf.X_HDR + layouts[r].q_cap:][:len(owned)].view(np.int32).tolist() == size[owned].tolist()
    n = 0
    for d in range(W):
        recv = np.concatenate([sends[s][d * bw:(d + 1) * bw] for s in range(W)])
        merged = bf.unpack_merge(layouts[d], recv, True)
        owned = list(range(d, nq, W))
        assert len(merged) == len(owned)
        for i, q in enumerate(owned):
            exp = {}
            for off, cnt, pid, km, fp, pos_off, bits in parts:
                w = bf.words_of(size[q])
                for t in range(int(off[q]), int(off[q + 1])):
                    a = exp.get(int(pid[t]), (0, 1 << 32, (0,) * w))
                    mine = bits[int(pos_off[t]):int(pos_off[t]) + w].tolist()
                    exp[int(pid[t])] = (a[0] + int(km[t]), min(a[1], int(fp[t])), tuple(x | y for x, y in zip(a[2], mine)))
            assert merged[i] == exp, (d, q)
            for k, f, words in exp.values():               # disjoint bitmaps: Kmatch = bits set, first position = lowest bit
                assert sum(bin(x).count("1") for x in words) == k and min(b for b in range(64 * len(words)) if words[b >> 6] >> (b & 63) & 1) == f
            n += len(exp)
    assert n > 100
    # the errors of the bitmap section
    recv = np.concatenate([sends[s][:bw] for s in range(W)])
    for word, value in ((bf.X_STATUS, int(recv[bw + bf.X_STATUS]) & ~bf.XS_BITMAPS), (bf.X_BITS_NEED, bf.p_cap(layouts[0]) + 1)):
        bad = recv.copy()
        bad[bw + word] = value
        with pytest.raises(ValueError):
            bf.unpack_merge(layouts[0], bad, True)
    bad = recv.copy()
    q0 = next(i for i in range(len(range(0, nq, W))) if size[i * W] > 1)
    bad[bw + bf.X_HDR + layouts[0].q_cap + q0] -= 1
    with pytest.raises(ValueError):
        bf.unpack_merge(layouts[0], bad, True)
    # a section too small for the bitmaps: the overflow bits, as for the entries
    tight = _layout(klib, 0, 64, 400, 1500, fit=(nq, 5 * nq, 4))
    off, cnt, pid, km, fp, pos_off, bits = parts[0]
    s = bf.pack_blocks(tight, nq, off, cnt, pid, km, fp, True, size=size, pos_off=pos_off, pos_bits=bits)
    tbw = int(tight.block_words)
    assert all(int(s[d * tbw + bf.X_STATUS]) & bf.XS_SENDER_OVERFLOW for d in range(W))
    assert any(int(s[d * tbw + bf.X_STATUS]) & bf.XS_OVERFLOW for d in range(W))
