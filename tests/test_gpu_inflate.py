"""The device inflate of BGZF blocks (inflate.hip.inc) against Python's zlib: every kind of deflate block, the sizes at which
the kernel's tiling changes, the match copy's store-then-load order, many blocks per call, and the malformed blocks that
tools/inflate_check has classified on the CPU -- each must end with its status word, the blocks beside it untouched, and
leave the inflater usable.  Also the cut rule on the device against kaamer_text_cut_fastq."""
import zlib

import numpy as np
import pytest

import bgzfmake
from kaamer_amd import api, workload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inflater(klib, gpu_device):
    inf = api.Inflater(1 << 22, 400, device=gpu_device)
    yield inf
    inf.close()


@pytest.fixture(scope="module")
def inflater_many(klib, gpu_device):
    """an inflater for calls of more blocks than the offsets scan has threads"""
    inf = api.Inflater(1 << 20, 3100, device=gpu_device)
    yield inf
    inf.close()


@pytest.fixture(scope="module")
def fastq(klib):
    return bytes(workload.fastq_text(workload.make_reads(workload.make_db(50), 1200, seed=9)))


def _inflate(inflater, data, out_offset=0):
    """(result, the blocks, what zlib makes of every block)"""
    blocks, used = api.bgzf_scan(data)
    assert used == len(data)
    want = [zlib.decompress(data[int(b["comp_off"]):int(b["comp_off"]) + int(b["comp_len"])], -15) if int(b["comp_len"]) else b"" for b in blocks]
    r = inflater.inflate(data, blocks, out_offset=out_offset)
    return r, blocks, want


def _assert_good(inflater, data, text, out_offset=0):
    r, blocks, want = _inflate(inflater, data, out_offset)
    assert b"".join(want) == text                               # (the fixture is what it claims to be)
    assert r["status"].tolist() == [0] * len(blocks) and r["n_bad"] == 0 and r["first_bad"] == 0xFFFFFFFF
    assert r["out_bytes"] == len(text)
    assert r["text"].tobytes() == text
    assert (r["guard"][0] == 0xEE).all() and (r["guard"][1] == 0xEE).all()     # nothing written outside the text


@pytest.mark.parametrize("mode", ["stored", "fixed", "level6", "level1", "level9_mem1", "huffman_only", "rle"])
def test_every_kind_of_deflate_block(inflater, fastq, mode):
    text = fastq[:65280]
    # (level9_mem1: memLevel 1 gives deflate a 128-symbol buffer, so the BGZF block holds hundreds of deflate blocks)
    _assert_good(inflater, bgzfmake.block(text, mode) + bgzfmake.EOF_BLOCK, text)


def test_sizes(inflater, fastq):
    seg = api.inflater_geometry()["crc_segment"]
    assert 65536 % seg == 0 and 65536 // seg <= 64
    for n in (0, 1, 2, seg - 1, seg, seg + 1, 2 * seg, 2 * seg + 1, 65280, 65535):
        for mode in ("level6", "stored") if n <= 65280 else ("level6",):       # (65 535 stored bytes do not fit a BGZF block)
            _assert_good(inflater, bgzfmake.block(fastq[:n], mode), fastq[:n], out_offset=3)
    a = b"A" * 65536                                            # length-258 matches at distance 1, and the largest block there is
    for mode in ("level6", "rle", "fixed"):
        _assert_good(inflater, bgzfmake.block(a, mode), a)
    noise = np.random.default_rng(2).integers(0, 256, 65280, dtype=np.uint8).tobytes()
    _assert_good(inflater, bgzfmake.block(noise, "level6"), noise)


def test_match_copy_reads_what_the_wave_just_stored(inflater):
    """period-k text: after the first k literals every match has distance k (or a multiple) and starts right behind bytes
    stored by the instruction before -- distances below, at and above the 64 lanes, lengths up to 258"""
    rng = np.random.default_rng(3)
    parts, texts = [], []
    for k in list(range(1, 71)) + [127, 128, 129, 257, 258, 259]:
        unit = rng.integers(97, 123, k, dtype=np.uint8).tobytes()
        for n in (700, 2051):
            t = (unit * (n // k + 1))[:n]
            parts.append(bgzfmake.block(t, "level9_mem1" if k % 2 else "level6"))
            texts.append(t)
    assert len(parts) <= 400
    _assert_good(inflater, b"".join(parts), b"".join(texts), out_offset=5)


def test_distance_32768(inflater):
    m, text = bgzfmake.distance_32768()
    _assert_good(inflater, m, text, out_offset=1)


@pytest.mark.parametrize("n_blocks", [1, 300])
def test_many_blocks_at_odd_offsets(inflater, fastq, n_blocks):
    rng = np.random.default_rng(n_blocks)
    modes = list(bgzfmake.MODES)
    pieces, at = [], 0
    for i in range(n_blocks):
        n = int(rng.integers(0, 900)) | 1 if i % 7 else 0       # odd sizes: no block but the first starts at a multiple of 16
        pieces.append(fastq[at:at + n])
        at += n
    assert at <= len(fastq)
    data = b"".join(bgzfmake.block(p, modes[i % len(modes)]) for i, p in enumerate(pieces))
    _assert_good(inflater, data, b"".join(pieces), out_offset=7)


def many_small_blocks(fastq, n_blocks):
    """(data, text, pieces): n_blocks BGZF blocks of 0 to 39 bytes of the fixture, every seventh empty, the modes in turn, and
    a last block of 40 bytes, the largest"""
    rng = np.random.default_rng(n_blocks)
    modes = list(bgzfmake.MODES)
    sizes = np.where(np.arange(n_blocks) % 7 == 0, 0, rng.integers(0, 40, n_blocks))
    sizes[-1] = 40
    ends = np.cumsum(sizes)
    assert ends[-1] <= len(fastq) and sizes.max() == sizes[-1] and (sizes[:-1] < sizes[-1]).all()
    pieces = [fastq[int(e - n):int(e)] for e, n in zip(ends, sizes)]
    data = b"".join(bgzfmake.block(p, modes[i % len(modes)]) for i, p in enumerate(pieces))
    return data, b"".join(pieces), pieces


def blocks_per_scan_thread(n_blocks):
    t = api.inflater_geometry()["scan_threads"]
    return (n_blocks + t - 1) // t


@pytest.mark.parametrize("n_blocks", [1024, 1025, 2047, 2048, 2049, 3001])
def test_more_blocks_than_scan_threads(inflater_many, fastq, n_blocks):
    """inf_offsets_kernel gives each of its 1024 threads ceil(n_blocks / 1024) blocks in a row: one at 1024; two from 1025
    on -- with 1025 blocks thread 512 holds the last block alone and the stretches of threads 513 to 1023 start behind
    it, with 2047 only thread 1023 is short (one block), 2048 fills every stretch; three at 2049 and 3001 (threads from
    683 resp. 1001 start behind the last block).  Every block's text lies where the sum of the sizes before it says."""
    t = api.inflater_geometry()["scan_threads"]
    assert t == 1024
    per = blocks_per_scan_thread(n_blocks)
    assert per == {1024: 1, 1025: 2, 2047: 2, 2048: 2, 2049: 3, 3001: 3}[n_blocks]
    idle = [k for k in range(t) if k * per >= n_blocks]             # threads whose stretch starts behind the last block
    if n_blocks == 1025:
        assert idle == list(range(513, 1024)) and 512 * per == n_blocks - 1
    if n_blocks == 2047:
        assert not idle and 1023 * per == n_blocks - 1
    if n_blocks in (1024, 2048):
        assert not idle and t * per == n_blocks
    if n_blocks == 2049:
        assert idle == list(range(683, 1024))
    assert n_blocks <= inflater_many.max_blocks
    data, text, _ = many_small_blocks(fastq, n_blocks)
    assert len(data) <= inflater_many.max_comp_bytes
    _assert_good(inflater_many, data, text, out_offset=7)


def test_malformed_block_behind_the_first_stretch(inflater_many, fastq):
    """two blocks per scan thread, and block 1024 -- the first of thread 512's stretch -- has a flipped CRC bit: its status,
    first_bad, and the text of every other block where the offsets put it"""
    n_blocks, bad_at = 1031, 1024
    assert blocks_per_scan_thread(n_blocks) == 2 and bad_at == api.inflater_geometry()["scan_threads"]
    data, text, pieces = many_small_blocks(fastq, n_blocks)
    blocks, used = api.bgzf_scan(data)
    assert used == len(data) and len(blocks) == n_blocks and len(pieces[bad_at]) > 0
    raw = bytearray(data)
    raw[int(blocks[bad_at + 1]["comp_off"]) - bgzfmake.HEADER - 8] ^= 1       # the CRC in block bad_at's trailer
    blocks2, used2 = api.bgzf_scan(bytes(raw))
    assert used2 == used and blocks2["crc"][bad_at] != blocks["crc"][bad_at] and (np.delete(blocks2["crc"], bad_at) == np.delete(blocks["crc"], bad_at)).all()
    r = inflater_many.inflate(bytes(raw), blocks2, out_offset=3)
    want_status = [0] * n_blocks
    want_status[bad_at] = 7
    assert r["status"].tolist() == want_status
    assert (r["n_bad"], r["first_bad"], r["first_bad_status"], r["out_bytes"]) == (1, bad_at, 7, len(text))
    a = sum(len(p) for p in pieces[:bad_at])
    b = a + len(pieces[bad_at])
    got = r["text"].tobytes()
    assert got[:a] == text[:a] and got[b:] == text[b:]
    assert got[a - len(pieces[bad_at - 1]):a] == pieces[bad_at - 1] and got[b:b + len(pieces[bad_at + 1])] == pieces[bad_at + 1]
    assert (r["guard"][0] == 0xEE).all() and (r["guard"][1] == 0xEE).all()
    _assert_good(inflater_many, data, text, out_offset=3)                     # the inflater is as good as new


def test_malformed_blocks_end_with_their_status(inflater, fastq):
    text = fastq[:2000]
    good = bgzfmake.block(text)
    payload = bgzfmake.deflate_raw(text)
    crc = bytearray(good)
    crc[-8] ^= 1
    cases = [
        (bytes(crc), 7),                                                     # a flipped bit of the trailer's CRC
        (bgzfmake.member(payload, text, isize=len(text) + 1), 6),            # ISIZE + 1: less output than stated
        (bgzfmake.member(payload, text, isize=len(text) - 1), 5),            # ISIZE - 1: more
        (bgzfmake.oversubscribed(), 2),
        (bgzfmake.distance_before_start(), 3),
        (bgzfmake.payload_cut_short(good), 4),
    ]
    other = fastq[3000:4500]
    for bad, status in cases:
        data = good + bad + bgzfmake.block(other)
        blocks, used = api.bgzf_scan(data)
        assert used == len(data) and len(blocks) == 3
        r = inflater.inflate(data, blocks, out_offset=2)
        assert r["status"].tolist() == [0, status, 0] and (r["n_bad"], r["first_bad"]) == (1, 1)
        # the good blocks around it are whole, and nothing was written outside the three blocks' bytes
        n1 = int(blocks[1]["isize"])
        assert r["text"][:len(text)].tobytes() == text and r["text"][len(text) + n1:].tobytes() == other
        assert (r["guard"][0] == 0xEE).all() and (r["guard"][1] == 0xEE).all()
        _assert_good(inflater, good + bgzfmake.EOF_BLOCK, text)             # the inflater is as good as new
    # a block table that points outside the compressed bytes of the call is refused, not read
    blocks, _ = api.bgzf_scan(good)
    blocks["comp_off"] = inflater.max_comp_bytes - 10
    r = inflater.inflate(good, blocks)
    assert r["status"].tolist() == [4]


def test_cut_on_the_device(klib, gpu_device):
    tile = api.inflater_geometry()["cut_tile"]
    rng = np.random.default_rng(4)
    base = bytearray(rng.choice(np.frombuffer(b"ACGTI+#", np.uint8), 3 * tile + 100).tobytes())
    for b in (tile, 2 * tile, 3 * tile, 16, 64 * 16):
        for p in (b - 1, b, b + 1):                              # the '\n' and the '@' on either side of a boundary
            t = bytearray(base)
            t[5:7] = b"\n@"                                      # an earlier cut that must lose
            t[p - 1:p + 1] = b"\n@"
            assert api.text_cut_fastq_device(bytes(t), gpu_device) == api.text_cut_fastq(bytes(t)) == p
    for t in (b"", b"@", b"\n", b"\n@", b"@r\nAC\n", bytes(base), b"x" * tile + b"\n", b"@" * (tile + 1)):
        assert api.text_cut_fastq_device(t, gpu_device) == api.text_cut_fastq(t)
    t = b"@a\nAC\n+\n@@II\n@b\nGT\n"
    assert api.text_cut_fastq_device(t, gpu_device) == api.text_cut_fastq(t) == 13
