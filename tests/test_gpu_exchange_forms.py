"""The exchange step's forms, pinned one by one (kaamer_exchange_pack / kaamer_exchange_merge, exchange.hip.inc).

Which scan runs (one workgroup per row with a carry, or the three tiled launches) is chosen by the layout's q_cap, and
which copy runs (a wave or 16 lanes per query) by the workspace's query capacity (pack) and by q_cap x world (merge) --
not by the batch.  So ONE batch of 2 x 8192 + 5 protein queries (every row of counts is longer than one tile, and the
items behind the tile boundary have hits) goes through every form at W = 2, both ranks on one card:

    the send blocks of every rank     == tests/blockfmt.py, bit for bit, on the words the format defines; the rest untouched
    the merged lists of every owner   == the unsharded Index.search(want_positions=True): hit set, Kmatch, first position, bitmap
    kaamer_exchange_stats(_positions) == the batch's query count, the largest [5] / [7] of the headers, no overflow

and the owner's verdicts over received headers that were changed on the way are today's errors, in both scan forms."""
import ctypes as C

import numpy as np
import pytest

import blockfmt as bf

W = 2
NQ = 2 * 8192 + 5
WIDE_QUERIES = 262144          # the copies take 16 lanes per query above this many queries
FILL = 0x5A5A5A5A              # what the send buffers hold before the pack

# form -> (queries the capacity layout is made for; 0: fitted to the batch, search workspace's query capacity)
FORMS = {
    "small-wide": (0, NQ),                                   # q_cap 8 196: two tiles in one workgroup, carry across them
    "tiled-wide": (80000, 80000),                            # q_cap 40 001: five tiles
    "tiled-narrow": (WIDE_QUERIES + 256, WIDE_QUERIES + 256),  # q_cap 131 201 per rank, x 2 > 262 144
    "small-narrow": (0, WIDE_QUERIES + 256),
}


def _dev(ptr, n, dtype):
    import torch
    from kaamer_amd import sharded
    t = {np.uint32: torch.int32, np.int32: torch.int32, np.uint64: torch.int64, np.uint8: torch.uint8}[dtype]
    return sharded.dev_tensor(ptr, int(n), t).cpu().numpy().view(dtype)


def _route(sends, layouts, d):
    """what rank d receives: block s = the block rank s packed for rank d (an all-to-all with equal splits)"""
    import torch
    bw = int(layouts[0].block_words)
    return torch.cat([sends[s][d * bw:(d + 1) * bw] for s in range(len(sends))])


def _canon(queries, hit_off, hit_cnt, pid, km, fp, size, pos_off, pos_bits):
    """per query, in protein-id order: [(pid, Kmatch, first position, bitmap words)]"""
    out = []
    for i in queries:
        a, n, w = int(hit_off[i]), int(hit_cnt[i]), bf.words_of(size[i])
        rows = []
        for t in range(a, a + n):
            bits = tuple(pos_bits[int(pos_off[t]):int(pos_off[t]) + w].tolist()) if pos_bits is not None else ()
            rows.append((int(pid[t]), int(km[t]), int(fp[t]) if fp is not None else 0, bits))
        out.append(sorted(rows))
    return out


class _World:
    """the batch, its unsharded result, and the W shard indexes"""

    def __init__(self, device):
        import torch
        from kaamer_amd import api, workload
        db = workload.make_db(600, seed=6)
        recs = workload.unpack(db)
        rng = np.random.default_rng(16)
        seqs = []
        for i in range(NQ):
            r = recs[int(rng.integers(0, len(recs)))]
            n = int(rng.integers(12, 41)) if i < NQ - 8 else int(rng.integers(20, 41))   # (12 residues: SizeInKmer 6, dropped)
            a = int(rng.integers(0, len(r) - n + 1))
            seqs.append(r[a:a + n])
        seqs[100], seqs[101] = b"", seqs[101][:6]
        self.buf, self.offs = api.pack_sequences(seqs)
        self.d_buf = torch.from_numpy(self.buf).cuda()
        self.d_off = torch.from_numpy(self.offs.view(np.int64)).cuda()
        ref = api.Index.from_image(api.Image.from_proteins(packed=db), device).search(packed=(self.buf, self.offs), want_positions=True)
        assert ref.n_queries == NQ
        self.size = ref.meta["size_in_kmer"].copy()
        assert self.size[100] == -6 and self.size[101] == 0 and ref.hit_cnt[100] == ref.hit_cnt[101] == 0
        assert all(ref.hit_cnt[q] > 0 for q in range(NQ - 8, NQ))       # the last items of both rows have hits
        self.ref = _canon(range(NQ), ref.hit_off, ref.hit_cnt, ref.hit_pid, ref.hit_kmatch, ref.hit_first_pos, self.size,
                          ref.pos_off, ref.pos_bits)
        self.ix = [api.Index.from_image(api.Image.from_proteins(packed=db, shard=r, n_shards=W), device) for r in range(W)]


@pytest.fixture(scope="module")
def world(klib, gpu_device):
    return _World(gpu_device)


class _Packed:
    """every rank's search of the batch, packed in one form: the partial lists (host), the layouts, the send blocks"""

    def __init__(self, world, form, arrays):
        import torch
        from kaamer_amd import abi, api
        self.world, self.arrays = world, arrays
        self.with_fp, self.bitmaps = arrays >= 3, arrays == 4
        self.fp_opt = 1 if self.with_fp else 2
        self.st = torch.cuda.current_stream()
        raw = self.st.cuda_stream
        layout_queries, ws_queries = FORMS[form]
        self.ws, self.parts = [], []
        for r in range(W):
            ws = api.Workspace(world.ix[r], len(world.buf), NQ, max_queries=ws_queries, first_pos=self.fp_opt, want_positions=self.bitmaps)
            assert ws.query_capacity == ws_queries
            res = ws.search_device(world.d_buf.data_ptr(), world.d_off.data_ptr(), NQ, len(world.buf), stream=raw)
            ws.finish(raw)
            assert int(_dev(res.d_n_queries, 1, np.uint32)[0]) == NQ
            hit_off, hit_cnt = _dev(res.d_hit_off, NQ, np.uint64).astype(np.int64), _dev(res.d_hit_cnt, NQ, np.uint32).astype(np.int64)
            nh = int((hit_off + hit_cnt).max())
            part = dict(hit_off=hit_off, hit_cnt=hit_cnt, pid=_dev(res.d_hit_pid, nh, np.uint32), km=_dev(res.d_hit_kmatch, nh, np.uint32),
                        fp=_dev(res.d_hit_first_pos, nh, np.uint32) if self.with_fp else None, size=None, pos_off=None, pos_bits=None)
            if self.bitmaps:
                part["size"] = _dev(res.d_q, NQ * api.META_DTYPE.itemsize, np.uint8).view(api.META_DTYPE)["size_in_kmer"].copy()
                assert part["size"].tolist() == world.size.tolist()
                part["pos_off"] = _dev(res.d_pos_off, nh, np.uint64).astype(np.int64)
                part["pos_bits"] = _dev(res.d_pos_bits, int(_dev(res.d_pos_base, NQ + 1, np.uint64)[NQ]), np.uint64)
            self.ws.append(ws)
            self.parts.append(part)
        # blocks with a little room to spare: what the largest (sender, owner) pair needs + 100
        self.need = max(int(p["hit_cnt"][d::W].sum()) for p in self.parts for d in range(W))
        self.pneed = max(int((p["hit_cnt"][d::W] * [bf.words_of(s) for s in world.size[d::W]]).sum()) for p in self.parts for d in range(W))
        L = abi.lib()
        self.layouts = []
        for r in range(W):
            cap, fit = abi.ExchangeLayout(), abi.ExchangeLayout()
            lq = layout_queries or ws_queries
            if self.bitmaps:
                abi.check(L.kaamer_exchange_layout_init_positions(W, r, lq, self.need + 100, self.pneed + 100, C.byref(cap)))
                abi.check(L.kaamer_exchange_layout_fit_positions(C.byref(cap), lq if layout_queries else NQ, self.need + 100, self.pneed + 100, C.byref(fit)))
            else:
                abi.check(L.kaamer_exchange_layout_init(W, r, lq, self.need + 100, C.byref(cap)))
                abi.check(L.kaamer_exchange_layout_fit(C.byref(cap), lq if layout_queries else NQ, self.need + 100, int(self.with_fp), C.byref(fit)))
            assert fit.arrays == arrays
            assert fit.q_cap == ((lq + W - 1) // W + 1 if layout_queries else (NQ + W - 1) // W + 1)
            self.layouts.append(fit)
        self.tiles = -(-int(self.layouts[0].q_cap) // 8192)
        self.sends = []
        for r in range(W):
            send = torch.full((W * int(self.layouts[r].block_words),), FILL, dtype=torch.int32, device="cuda")
            self.ws[r].exchange_pack(self.layouts[r], send.data_ptr(), raw)
            self.sends.append(send)
        self.st.synchronize()

    def merge_workspace(self, d):
        from kaamer_amd import api
        L = self.layouts[d]
        return api.Workspace(self.world.ix[d], 64, L.q_cap, max_queries=L.q_cap, first_pos=self.fp_opt, max_hits=W * int(L.e_cap),
                             want_positions=self.bitmaps, max_pos_words=W * bf.p_cap(L))

    def expected(self, d):
        """the unsharded lists of the queries rank d owns, as a merge with this form's arrays returns them"""
        return [[(p, k, f if self.with_fp else 0, b if self.bitmaps else ()) for p, k, f, b in rows] for rows in self.world.ref[d::W]]

    def merged(self, d, m):
        n = len(range(d, NQ, W))
        hit_off, hit_cnt = _dev(m.d_hit_off, n, np.uint64).astype(np.int64), _dev(m.d_hit_cnt, n, np.uint32).astype(np.int64)
        nh = int((hit_off + hit_cnt).max())
        pos_off = _dev(m.d_pos_off, nh, np.uint64).astype(np.int64) if self.bitmaps else None
        pos_bits = _dev(m.d_pos_bits, int(_dev(m.d_pos_base, n + 1, np.uint64)[n]), np.uint64) if self.bitmaps else None
        return _canon(range(n), hit_off, hit_cnt, _dev(m.d_hit_pid, nh, np.uint32), _dev(m.d_hit_kmatch, nh, np.uint32),
                      _dev(m.d_hit_first_pos, nh, np.uint32), self.world.size[d::W], pos_off, pos_bits)


CASES = [(f, 4) for f in FORMS] + [(f, a) for f in ("small-wide", "tiled-wide") for a in (3, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,arrays", CASES, ids=["%s-%d" % c for c in CASES])
def test_exchange_form(klib, gpu_device, world, form, arrays):
    px = _Packed(world, form, arrays)
    assert (px.tiles <= 4) == form.startswith("small") and px.tiles >= 2
    raw = px.st.cuda_stream
    # ---- the send blocks, bit for bit
    hdr_need = hdr_pneed = 0
    for r in range(W):
        p, L = px.parts[r], px.layouts[r]
        got = px.sends[r].cpu().numpy().view(np.uint32)
        exp = bf.pack_blocks(L, NQ, p["hit_off"], p["hit_cnt"], p["pid"], p["km"], p["fp"], px.with_fp, size=p["size"],
                             pos_off=p["pos_off"], pos_bits=p["pos_bits"])
        m = bf.defined_words(L, exp, px.with_fp)
        bad = np.flatnonzero(got[m] != exp[m])
        assert len(bad) == 0, (r, np.flatnonzero(m)[bad][:8].tolist())
        assert (got[~m] == FILL).all(), r
        bw = int(L.block_words)
        for d in range(W):
            h = got[d * bw:d * bw + bf.X_HDR]
            assert h[bf.X_STATUS] == (bf.XS_FIRST_POS if px.with_fp else 0) | (bf.XS_BITMAPS if px.bitmaps else 0), (r, d)
            assert h[bf.X_NQ] == NQ and h[bf.X_ENTRIES] == h[bf.X_NEED] == int(p["hit_cnt"][d::W].sum()) > 8192
        hdr_need, hdr_pneed = max(hdr_need, int(got[bf.X_NEED_MAX])), max(hdr_pneed, int(got[bf.X_BITS_NEED_MAX]))
    assert hdr_need == px.need and hdr_pneed == (px.pneed if px.bitmaps else 0)
    # ---- route, merge on each owner, against the unsharded search
    n_checked = 0
    for d in range(W):
        mws = px.merge_workspace(d)
        recv = _route(px.sends, px.layouts, d)
        m = mws.exchange_merge(px.layouts[d], recv.data_ptr(), raw)
        c = mws.finish(raw)
        assert mws.exchange_stats(0) == (0, NQ, hdr_need, 0)
        assert mws.exchange_stats_positions(0) == (hdr_pneed, 0)
        assert int(_dev(m.d_n_queries, 1, np.uint32)[0]) == len(range(d, NQ, W))
        got, exp = px.merged(d, m), px.expected(d)
        for i, (a, b) in enumerate(zip(got, exp)):
            assert a == b, (d, d + i * W)
        n_checked += sum(len(x) for x in exp)
        assert c["n_hits"] == sum(len(x) for x in exp)
        mws.close()
    assert n_checked > 4 * 8192
    for ws in px.ws:
        ws.close()


# ---- the owner's verdicts ----------------------------------------------------------------------------------------------
CAP_MSG, PEER_MSG = "exchange block capacity exceeded", "a peer's search of this batch exceeded"
# case -> (message of kaamer_workspace_finish, `overflow` of kaamer_exchange_stats, of kaamer_exchange_stats_positions)
VERDICTS = {
    "nq-differs": (CAP_MSG, 0, 0),
    "overflow-bit": (CAP_MSG, 1, 0),
    "sender-overflow-bit-alone": (CAP_MSG, 1, 0),
    "sender-failed-bit": (PEER_MSG, 0, 0),
    "first-pos-bit-cleared": (CAP_MSG, 1, 0),
    "bitmaps-bit-cleared": (CAP_MSG, 0, 0),
    "bitmap-need-above-section": (CAP_MSG, 0, 1),
    "size-smaller-in-one-source": (CAP_MSG, 0, 0),
}


@pytest.fixture(scope="module", params=["small-wide", "tiled-wide"])
def packed4(request, world):
    px = _Packed(world, request.param, 4)
    px.mws = px.merge_workspace(0)
    px.n_merges = 0
    yield px
    px.mws.close()
    for ws in px.ws:
        ws.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(VERDICTS))
def test_owner_verdict(klib, gpu_device, world, packed4, case):
    """rank 0 receives rank 1's block with ONE header word (or one SizeInKmer word) changed: no count word is touched, so
    every offset the kernels derive stays inside the buffers; the merge is refused, and the next one on the same workspace
    is clean"""
    import torch
    from kaamer_amd import abi
    px, L = packed4, packed4.layouts[0]
    raw, bw = px.st.cuda_stream, int(L.block_words)
    good = _route(px.sends, px.layouts, 0)
    blocks = good.cpu().numpy().view(np.uint32).copy()
    b1 = blocks[bw:2 * bw]                      # what rank 1 sent
    assert b1[bf.X_STATUS] == bf.XS_FIRST_POS | bf.XS_BITMAPS
    if case == "nq-differs":
        b1[bf.X_NQ] += 1
    elif case == "overflow-bit":
        b1[bf.X_STATUS] |= bf.XS_OVERFLOW
    elif case == "sender-overflow-bit-alone":
        b1[bf.X_STATUS] |= bf.XS_SENDER_OVERFLOW
    elif case == "sender-failed-bit":
        b1[bf.X_STATUS] |= bf.XS_SENDER_FAILED
    elif case == "first-pos-bit-cleared":
        b1[bf.X_STATUS] &= ~np.uint32(bf.XS_FIRST_POS)
    elif case == "bitmaps-bit-cleared":
        b1[bf.X_STATUS] &= ~np.uint32(bf.XS_BITMAPS)
    elif case == "bitmap-need-above-section":
        b1[bf.X_BITS_NEED] = bf.p_cap(L) + 1
    else:
        sizes = b1[bf.X_HDR + L.q_cap:bf.X_HDR + L.q_cap + 8195]
        # an owned query behind the tile boundary, with hits in this block
        i = next(j for j in range(8192, 8195) if b1[bf.X_HDR + j] > 0 and 8 <= sizes[j] <= 64)
        sizes[i] -= 1                           # (one bitmap word before and after: the offsets stay what they were)
    bad = torch.from_numpy(blocks.view(np.int32)).cuda()
    msg, ovf, povf = VERDICTS[case]
    px.mws.exchange_merge(L, bad.data_ptr(), raw)
    with pytest.raises(abi.KaamerError) as e:
        px.mws.finish(raw)
    assert e.value.code == abi.E_CAPACITY and msg in str(e.value), str(e.value)
    seq, nq, need, got_ovf = px.mws.exchange_stats(0)
    assert (seq, nq, need, got_ovf) == (px.n_merges, NQ, px.need, ovf)
    assert px.mws.exchange_stats_positions(0) == (px.pneed, povf)
    # the same workspace, the blocks as they were sent
    m = px.mws.exchange_merge(L, good.data_ptr(), raw)
    c = px.mws.finish(raw)
    px.n_merges += 2
    assert px.mws.exchange_stats(0) == (px.n_merges - 1, NQ, px.need, 0) and px.mws.exchange_stats_positions(0) == (px.pneed, 0)
    exp = px.expected(0)
    assert c["n_hits"] == sum(len(x) for x in exp)
    if case == "size-smaller-in-one-source":    # once per form: the whole result after a refused merge
        assert px.merged(0, m) == exp
