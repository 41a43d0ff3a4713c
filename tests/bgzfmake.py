"""BGZF fixtures for the tests: deflate payloads from Python's zlib (or made by hand, bit by bit) wrapped in BGZF headers and
trailers.  A BGZF member is 1f 8b 08 04 MTIME(4) XFL OS XLEN(2) [subfields] | deflate | CRC32 ISIZE, the subfield B C 2 0
holding BSIZE = the member's size - 1."""
import struct
import zlib

import numpy as np

# (level, memLevel, strategy): stored, level 1, fixed codes only, many deflate blocks per BGZF block, Huffman only, RLE
MODES = {
    "stored": (0, 8, zlib.Z_DEFAULT_STRATEGY),
    "level1": (1, 8, zlib.Z_DEFAULT_STRATEGY),
    "fixed": (6, 8, zlib.Z_FIXED),
    "level9_mem1": (9, 1, zlib.Z_DEFAULT_STRATEGY),
    "huffman_only": (6, 8, zlib.Z_HUFFMAN_ONLY),
    "rle": (6, 8, zlib.Z_RLE),
    "level6": (6, 8, zlib.Z_DEFAULT_STRATEGY),
}
HEADER = 18   # bytes of a member's header when BC is its only subfield


def deflate_raw(text, mode="level6"):
    level, mem, strategy = MODES[mode]
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(bytes(text)) + c.flush()


def member(payload, text, pre_extra=b"", flg=4, isize=None, crc=None):
    """one BGZF member around a deflate payload; pre_extra: raw subfields in front of BC"""
    text = bytes(text)
    xlen = len(pre_extra) + 6
    bsize = 12 + xlen + len(payload) + 8 - 1
    assert bsize < 65536
    head = struct.pack("<BBBBIBBH", 0x1F, 0x8B, 8, flg, 0, 0, 0xFF, xlen) + pre_extra + struct.pack("<BBHH", 66, 67, 2, bsize)
    return head + payload + struct.pack("<II", zlib.crc32(text) if crc is None else crc, len(text) if isize is None else isize)


def block(text, mode="level6", **kw):
    return member(deflate_raw(text, mode), text, **kw)


EOF_BLOCK = block(b"")


def bgzf_file(text, block_bytes, mode="level6", eof=True):
    """`text` as bgzip writes it: blocks of block_bytes of text each, then the empty end-of-file block"""
    text = bytes(text)
    parts = [block(text[i:i + block_bytes], mode) for i in range(0, len(text), block_bytes)]
    return b"".join(parts) + (EOF_BLOCK if eof else b"")


class BitWriter:
    """deflate's bit order: fields from the least significant bit of each byte up, Huffman codes most significant bit first"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, k):
        for i in range(k):
            self.acc |= ((v >> i) & 1) << self.n
            self.n += 1
            if self.n == 8:
                self.out.append(self.acc)
                self.acc, self.n = 0, 0
        return self

    def code(self, v, k):
        for i in reversed(range(k)):
            self.bits((v >> i) & 1, 1)
        return self

    def align(self):
        if self.n:
            self.out.append(self.acc)
            self.acc, self.n = 0, 0
        return self

    def raw(self, data):
        assert self.n == 0
        self.out += data
        return self


def distance_32768():
    """(member, text): 32 768 stored bytes, then a fixed-code block with one match of 258 bytes at distance 32 768 -- the
    longest distance there is; zlib's own deflate stops 262 bytes short of it"""
    head = np.random.default_rng(5).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = BitWriter()
    w.bits(0, 1).bits(0, 2).align().bits(32768, 16).bits(32768 ^ 0xFFFF, 16).raw(head)
    w.bits(1, 1).bits(1, 2).code(0xC0 + 5, 8).code(29, 5).bits(32768 - 24577, 13).code(0, 7).align()
    text = head + head[:258]
    assert zlib.decompress(bytes(w.out), -15) == text
    return member(bytes(w.out), text), text


def oversubscribed():
    """a dynamic block whose 19 code-length codes all have length 1"""
    w = BitWriter()
    w.bits(1, 1).bits(2, 2).bits(0, 5).bits(0, 5).bits(15, 4)
    for _ in range(19):
        w.bits(1, 3)
    return member(bytes(w.align().out), b"AAAA")


def distance_before_start():
    """a fixed-code block: the literal 'A', then a match of 3 bytes at distance 2"""
    w = BitWriter()
    w.bits(1, 1).bits(1, 2).code(0x30 + 65, 8).code(1, 7).code(1, 5).code(0, 7).align()
    return member(bytes(w.out), b"AAAA")


def payload_cut_short(m, n=5):
    """the member with the last n bytes of its payload gone and BSIZE following (the scan still takes it)"""
    m = bytearray(m[:-8 - n] + m[-8:])
    m[16:18] = struct.pack("<H", len(m) - 1)
    return bytes(m)
