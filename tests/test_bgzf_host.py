"""kaamer_bgzf_scan: the blocks of a BGZF stream found on the host without inflating (include/kaamer_hip.h).  CPU only."""
import gzip
import struct
import zlib

import numpy as np
import pytest

import bgzfmake
from kaamer_amd import api, workload


@pytest.fixture(scope="module")
def text(klib):
    db = workload.make_db(50)
    t = bytes(workload.fastq_text(workload.make_reads(db, 3000, seed=3)))
    assert len(t) >= 6 * 65280
    return t


def _check_blocks(data, blocks, pieces):
    """every block's payload inflates (zlib) to its piece of the text, and the record repeats the trailer"""
    assert len(blocks) == len(pieces)
    for b, piece in zip(blocks, pieces):
        off, n = int(b["comp_off"]), int(b["comp_len"])
        assert zlib.decompress(data[off:off + n], -15) == piece
        assert int(b["isize"]) == len(piece) and int(b["crc"]) == zlib.crc32(piece)
        assert struct.unpack("<II", data[off + n:off + n + 8]) == (zlib.crc32(piece), len(piece))


def test_six_kinds_of_block_and_the_eof_block(text):
    modes = ["stored", "level1", "fixed", "level9_mem1", "huffman_only", "rle"]
    pieces = [text[i * 65280:(i + 1) * 65280] for i in range(6)]
    data = b"".join(bgzfmake.block(p, m) for p, m in zip(pieces, modes)) + bgzfmake.EOF_BLOCK
    assert gzip.decompress(data) == b"".join(pieces)            # a valid multi-member gzip file
    assert len(bgzfmake.EOF_BLOCK) == 28
    blocks, used = api.bgzf_scan(data)
    assert used == len(data)
    _check_blocks(data, blocks, pieces + [b""])
    assert int(blocks[-1]["isize"]) == 0 and int(blocks[-1]["comp_len"]) == 2
    assert int(blocks[0]["comp_off"]) == bgzfmake.HEADER
    # incompressible bytes at level 6: a 65 326-byte member, inside the format's limit
    noise = np.random.default_rng(1).integers(0, 256, 65280, dtype=np.uint8).tobytes()
    m = bgzfmake.block(noise, "level6")
    assert 65280 < len(m) <= 65536
    blocks, used = api.bgzf_scan(m)
    assert used == len(m)
    _check_blocks(m, blocks, [noise])


def test_small_blocks_as_bgzip_writes_them(text):
    text = text[:50000]
    data = bgzfmake.bgzf_file(text, 700)
    blocks, used = api.bgzf_scan(data)
    assert used == len(data) and len(blocks) == -(-50000 // 700) + 1
    _check_blocks(data, blocks, [text[i:i + 700] for i in range(0, 50000, 700)] + [b""])
    assert api.bgzf_scan(b"")[1] == 0 and len(api.bgzf_scan(b"")[0]) == 0


def test_a_subfield_before_bc(text):
    piece = text[:1000]
    for pre in (b"XY\x03\x00abc", b"BC\x03\x00abc", b"AB\x00\x00" + b"CD\x01\x00z"):   # (a BC of another length is not the BGZF subfield)
        m = bgzfmake.block(piece, pre_extra=pre)
        assert gzip.decompress(m) == piece
        blocks, used = api.bgzf_scan(m + bgzfmake.EOF_BLOCK)
        assert used == len(m) + 28 and int(blocks[0]["comp_off"]) == bgzfmake.HEADER + len(pre)
        _check_blocks(m + bgzfmake.EOF_BLOCK, blocks, [piece, b""])


def test_where_the_scan_stops(text):
    good = bgzfmake.block(text[:900])
    piece = text[900:2000]

    def stops_after_first(tail):
        blocks, used = api.bgzf_scan(good + tail)
        assert (len(blocks), used) == (1, len(good))

    stops_after_first(bgzfmake.block(piece, flg=0))                      # FLG != 4: no extra field announced
    stops_after_first(bgzfmake.block(piece, flg=4 | 8))                  # FNAME set as well
    stops_after_first(gzip.compress(piece))                             # ordinary gzip
    stops_after_first(bgzfmake.block(piece)[:-1])                        # cut short by one byte
    stops_after_first(bgzfmake.block(piece)[:10])                        # ... inside the header
    stops_after_first(bgzfmake.block(piece, isize=65537))                # ISIZE beyond a BGZF block
    stops_after_first(b"\x1f\x8b\x08\x04" + b"\0" * 6 + b"\x06\x00XY\x02\x00\x00\x00" + b"\0" * 40)   # no BC subfield
    stops_after_first(b"\x1f\x8b\x08\x04" + b"\0" * 6 + b"\x06\x00BC\x02\x00\x10\x00" + b"\0" * 40)   # BSIZE + 1 = 17 < header + trailer
    stops_after_first(b"\x1f\x8b\x08\x04" + b"\0" * 6 + b"\x06\x00XY\x09\x00\x00\x00" + b"\0" * 40)   # a subfield that leaves the extra field
    stops_after_first(b"@r1\nACGT\n")
    # ISIZE of exactly 65536 is a block
    full = bgzfmake.block(b"A" * 65536)
    blocks, used = api.bgzf_scan(full)
    assert used == len(full) and int(blocks[0]["isize"]) == 65536
    # ordinary gzip from the first byte on: nothing
    blocks, used = api.bgzf_scan(gzip.compress(piece))
    assert (len(blocks), used) == (0, 0)
