"""numpy restatement of the sharded exchange's fixed-size block format (kaamer_amd/csrc/exchange.hip.inc), test
infrastructure only.  Rank r sends one block of `block_words` u32 words to every rank d:

    [0] entries in the block   [1] status (bit 0: capacity exceeded, bit 1: first positions inside, bit 2: sender failed,
                                   bit 3: some block of this sender exceeded its capacity, bit 4: bitmaps inside)
    [2] queries of the batch   [3] queries owned by d = ceil((nq - d) / W)
    [4] entries the block needed   [5] the largest [4] over the sender's W blocks
    [6] bitmap words the block needed   [7] the largest [6] over the sender's W blocks   (zero without bitmaps)
    [8 .. 8+q_cap)             per owned query i (global query d + i W): number of entries
    then pid[e_cap], kmatch[e_cap], first_pos[e_cap]

Blocks with PositionHits bitmaps (layout.arrays = 4) hold SizeInKmer[q_cap] after the counts (the entry arrays follow it)
and, from the even word bits_off = 8 + 2 q_cap + 3 e_cap (rounded up), p_cap = (block_words - bits_off) / 2 u64 words:
entry j of owned query i has w_i = ceil(SizeInKmer_i / 64) words at bbase[i] + j w_i, bbase = the scan of entries_i x w_i.

The names of the header words and status bits are the device file's (X_ENTRIES ..., XS_OVERFLOW ...).
`defined_words` lists the words of a block the format defines (the device leaves the rest of a block untouched), so a
device block and a numpy block can be compared bit for bit."""
import numpy as np

X_HDR = 8
# header words
X_ENTRIES, X_STATUS, X_NQ, X_OWNED, X_NEED, X_NEED_MAX, X_BITS_NEED, X_BITS_NEED_MAX = range(8)
# status bits
XS_OVERFLOW, XS_FIRST_POS, XS_SENDER_FAILED, XS_SENDER_OVERFLOW, XS_BITMAPS = 1, 2, 4, 8, 16


def _geom(layout):
    return int(layout.world), int(layout.q_cap), int(layout.e_cap), int(layout.block_words)


def has_bitmaps(layout):
    return int(layout.arrays) == 4


def ent_base(layout):
    """u32 word of a block at which the entry arrays start"""
    return X_HDR + (2 if has_bitmaps(layout) else 1) * int(layout.q_cap)


def bits_off(layout):
    """u32 word of a block at which the bitmap section starts (arrays = 4)"""
    return (X_HDR + 2 * int(layout.q_cap) + 3 * int(layout.e_cap) + 1) & ~1


def p_cap(layout):
    """u64 words of a block's bitmap section"""
    return max(0, (int(layout.block_words) - bits_off(layout)) // 2) if has_bitmaps(layout) else 0


def words_of(size):
    """u64 words of one bitmap of a query with this SizeInKmer (as int32)"""
    size = int(np.int32(np.uint32(int(size) & 0xFFFFFFFF)))
    return (size + 63) >> 6 if size > 0 else 0


def _bits64(blk, layout):
    o = bits_off(layout)
    return blk[o:o + 2 * p_cap(layout)].view(np.uint64)


def pack_blocks(layout, nq, hit_off, hit_cnt, pid, km, fp, with_fp, src_status=0, size=None, pos_off=None, pos_bits=None):
    """partial hit lists of ALL nq queries of one rank -> world blocks (one flat uint32 array).  arrays = 4: size[nq]
    (SizeInKmer), pos_off (per hit: first word of its bitmap in pos_bits) and pos_bits (uint64)"""
    W, q_cap, e_cap, bw = _geom(layout)
    bitmaps = has_bitmaps(layout)
    eb, pc = ent_base(layout), p_cap(layout)
    out = np.zeros(W * bw, np.uint32)
    for d in range(W):
        blk = out[d * bw:(d + 1) * bw]
        owned = list(range(d, nq, W))
        st = 0
        if len(owned) > q_cap:
            owned, st = owned[:q_cap], XS_OVERFLOW
        cnt = np.array([int(hit_cnt[q]) for q in owned], np.int64)
        total = int(cnt.sum())
        blk[X_HDR:X_HDR + len(owned)] = cnt
        if total > e_cap:
            st, total_w = XS_OVERFLOW, 0
        else:
            total_w = total
            o = 0
            ent = blk[eb:]
            for q, n in zip(owned, cnt):
                s = int(hit_off[q])
                ent[o:o + n] = pid[s:s + n]
                ent[e_cap + o:e_cap + o + n] = km[s:s + n]
                if with_fp:
                    ent[2 * e_cap + o:2 * e_cap + o + n] = fp[s:s + n]
                o += int(n)
        blk[X_ENTRIES] = total_w
        blk[X_STATUS] = st | (XS_FIRST_POS if with_fp else 0) | (XS_SENDER_FAILED if src_status else 0)
        blk[X_NQ] = nq
        blk[X_OWNED] = len(owned)
        blk[X_NEED] = min(total, 0xFFFFFFFF)
        if bitmaps:
            w = np.array([words_of(size[q]) for q in owned], np.int64)
            blk[X_HDR + q_cap:X_HDR + q_cap + len(owned)] = np.array([int(size[q]) & 0xFFFFFFFF for q in owned], np.uint32)
            need = int((cnt * w).sum())
            blk[X_BITS_NEED] = min(need, 0xFFFFFFFF)
            blk[X_STATUS] |= XS_BITMAPS | (XS_OVERFLOW if need > pc else 0)
            if need <= pc and not src_status:   # (a failed search sends no bitmaps)
                bits, o = _bits64(blk, layout), 0
                for q, n, wq in zip(owned, cnt, w):
                    s = int(hit_off[q])
                    if n and wq:   # hit j of the query: its wq words at o + j wq
                        first = np.asarray(pos_off[s:s + n]).astype(np.int64)
                        bits[o:o + n * wq] = pos_bits[(first[:, None] + np.arange(wq)).ravel()]
                    o += int(n * wq)
    for word, word_max in ((X_NEED, X_NEED_MAX),) + (((X_BITS_NEED, X_BITS_NEED_MAX),) if bitmaps else ()):
        out[word_max::bw] = max(int(out[d * bw + word]) for d in range(W))
    if any(int(out[d * bw + X_STATUS]) & XS_OVERFLOW for d in range(W)):
        out[X_STATUS::bw] |= XS_SENDER_OVERFLOW
    return out


def defined_words(layout, blocks, with_fp):
    """boolean mask over `blocks` (world blocks) of the words the format defines"""
    W, q_cap, e_cap, bw = _geom(layout)
    bitmaps = has_bitmaps(layout)
    m = np.zeros(W * bw, bool)
    for d in range(W):
        blk = blocks[d * bw:(d + 1) * bw]
        n_ent, n_owned = int(blk[X_ENTRIES]), min(int(blk[X_OWNED]), q_cap)
        b = d * bw
        m[b:b + X_HDR + n_owned] = True
        if bitmaps:
            m[b + X_HDR + q_cap:b + X_HDR + q_cap + n_owned] = True
            if int(blk[X_BITS_NEED]) <= p_cap(layout) and not int(blk[X_STATUS]) & XS_SENDER_FAILED:
                m[b + bits_off(layout):b + bits_off(layout) + 2 * int(blk[X_BITS_NEED])] = True
        e0 = b + ent_base(layout)
        for a in range(3 if with_fp else 2):
            m[e0 + a * e_cap:e0 + a * e_cap + n_ent] = True
    return m


def unpack_merge(layout, recv, with_fp):
    """received blocks (block s = what rank s packed for this rank) -> per owned query {pid: (Kmatch sum, lowest first
    position)}, and with arrays = 4 {pid: (Kmatch sum, lowest first position, OR of the bitmaps as a tuple of u64 words)};
    raises ValueError where the device reports an error (overflowed block, sender failed, missing first positions or
    bitmaps, headers or sizes that do not describe one batch)"""
    W, q_cap, e_cap, bw = _geom(layout)
    rank, bitmaps = int(layout.rank), has_bitmaps(layout)
    blks = [recv[s * bw:(s + 1) * bw] for s in range(W)]
    nq = int(blks[0][X_NQ])
    want = len(range(rank, nq, W))
    for b in blks:
        if int(b[X_NQ]) != nq or int(b[X_OWNED]) != want or want > q_cap:
            raise ValueError("headers disagree")
        if int(b[X_STATUS]) & (XS_OVERFLOW | XS_SENDER_OVERFLOW):
            raise ValueError("block overflow")
        if int(b[X_STATUS]) & XS_SENDER_FAILED:
            raise ValueError("peer failed")
        if with_fp and not int(b[X_STATUS]) & XS_FIRST_POS:
            raise ValueError("first positions missing")
        if bitmaps and not int(b[X_STATUS]) & XS_BITMAPS:
            raise ValueError("bitmaps missing")
        if bitmaps and max(int(b[X_BITS_NEED]), int(b[X_BITS_NEED_MAX])) > p_cap(layout):
            raise ValueError("bitmap section overflow")
        if bitmaps and not np.array_equal(b[X_HDR + q_cap:X_HDR + q_cap + want], blks[0][X_HDR + q_cap:X_HDR + q_cap + want]):
            raise ValueError("sizes disagree")
    out = [dict() for _ in range(want)]
    for b in blks:
        cnt = b[X_HDR:X_HDR + want].astype(np.int64)
        ent = b[ent_base(layout):]
        bits = _bits64(b, layout) if bitmaps else None
        o = bo = 0
        for i, n in enumerate(cnt):
            w = words_of(b[X_HDR + q_cap + i]) if bitmaps else 0
            for t in range(o, o + int(n)):
                p, k = int(ent[t]), int(ent[e_cap + t])
                f = int(ent[2 * e_cap + t]) if with_fp else 0
                if bitmaps:
                    a = out[i].get(p, (0, 1 << 32, (0,) * w))
                    mine = bits[bo + (t - o) * w:bo + (t - o + 1) * w].tolist()
                    out[i][p] = (a[0] + k, min(a[1], f), tuple(x | y for x, y in zip(a[2], mine)))
                else:
                    a = out[i].get(p, (0, 1 << 32))
                    out[i][p] = (a[0] + k, min(a[1], f))
            o += int(n)
            bo += int(n) * w
    return out
