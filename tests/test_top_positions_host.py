"""CPU-side checks of the PositionHits-for-reported-hits feature: the new symbols are declared and exported, the ABI
version did not move, and kaamer_format_positions is FormatPositionsToString (pkg/search/search.go:694-742) byte for
byte.  No device calls here."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_ONLY = bool(os.environ.get("KAAMER_HOST_ONLY"))   # the sanitized CPU build holds the host sources only
KMER_SIZE = 7

NEW_SYMBOLS = ["kaamer_topn_positions_device", "kaamer_search_batch_top_pos_flat", "kaamer_submit_batch_top_pos_flat",
               "kaamer_stream_open_pos_flat", "kaamer_batch_top_positions", "kaamer_format_positions"]


def format_positions_ref(positions, with_alignment):
    """search.go:694-742, restated line by line (dead branch included)"""
    current_start = 0
    in_sequence = False
    end_pos = 0
    s = ""
    for pos, match in enumerate(positions):
        if match:
            if not in_sequence:
                current_start = pos + 1
                in_sequence = True
        else:
            if in_sequence:
                if pos + 1 > current_start:
                    if s != "":
                        s += ","
                    end_pos = pos + 1
                    if with_alignment:
                        end_pos = end_pos + KMER_SIZE - 1
                    s += str(current_start) + "-" + str(end_pos)
                    in_sequence = False
                else:
                    if s != "":
                        s += ","
                    s += str(current_start)
                    in_sequence = False
    if in_sequence:
        if s != "":
            s += ","
        end_pos = len(positions)
        if with_alignment:
            end_pos = end_pos + KMER_SIZE - 1
        s += str(current_start) + "-" + str(end_pos)
    return s


def pack_bits(positions):
    positions = np.asarray(positions, dtype=bool)
    n = len(positions)
    padded = np.zeros(((n + 63) // 64) * 64, np.uint8)
    padded[:n] = positions
    return np.packbits(padded, bitorder="little").view(np.uint64) if n else np.zeros(0, np.uint64)


def format_lib(klib, positions, with_alignment):
    words = pack_bits(positions)
    ptr = words.ctypes.data if len(words) else None
    need = klib.kaamer_format_positions(ptr, len(positions), int(with_alignment), None, 0)
    buf = C.create_string_buffer(int(need) + 1)
    got = klib.kaamer_format_positions(ptr, len(positions), int(with_alignment), buf, need + 1)
    assert got == need
    assert len(buf.value) == need
    return buf.value.decode()


def test_new_symbols_declared_and_abi_version_unchanged():
    from kaamer_amd import abi
    src = open(os.path.join(ROOT, "include", "kaamer_hip.h")).read()
    assert re.search(r"#define\s+KAAMER_ABI_VERSION\s+4\b", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(kaamer_[a-z_0-9]+)\s*\(", code))
    for n in NEW_SYMBOLS:
        assert n in declared, "include/kaamer_hip.h does not declare %s" % n
        assert n in abi.SYMBOLS, "abi.py does not bind %s" % n


@pytest.mark.skipif(HOST_ONLY, reason="host-only sanitized library")
def test_new_symbols_exported(klib):
    for n in NEW_SYMBOLS:
        assert hasattr(klib, n), "libkaamer_hip.so lacks %s" % n
    assert klib.kaamer_abi_version() == 4


def test_existing_struct_sizes_unchanged():
    """additive only: the structs a caller allocates keep their size"""
    from kaamer_amd import abi
    assert C.sizeof(abi.BatchTop) == 80 + C.sizeof(abi.Counters)
    assert C.sizeof(abi.TopnResult) == 64
    assert C.sizeof(abi.TopnOpts) == 48
    assert C.sizeof(abi.WorkspaceOpts) == 64


@pytest.mark.parametrize("with_alignment", [False, True])
def test_format_positions_fixed_cases(klib, with_alignment):
    add = KMER_SIZE - 1 if with_alignment else 0
    cases = [[], [False] * 10, [True] * 264, [True], [False, True], [True, False], [False] * 5 + [True] + [False] * 5,
             [False] * 60 + [True] * 4, [True, False] * 40]
    for n in (63, 64, 65, 129):
        cases.append([True] * n)
        cases.append([False] * (n - 1) + [True])          # a run ending at the last position
        cases.append([True] + [False] * (n - 2) + [True])
        cases.append([(i % 64) in (0, 62, 63) for i in range(n)])   # runs across word boundaries
    for c in cases:
        assert format_lib(klib, c, with_alignment) == format_positions_ref(c, with_alignment), c
    assert format_lib(klib, [], with_alignment) == ""
    assert format_lib(klib, [False] * 10, with_alignment) == ""
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "docs_example.json")))
    text = json.dumps(doc)
    assert "264" in text   # the docs example: n_positions 264, all positions true
    assert format_lib(klib, [True] * 264, with_alignment) == "1-%d" % (264 + add)
    # the reference's odd corner: a closed run prints one past its last set position
    assert format_lib(klib, [False] * 5 + [True] + [False] * 5, with_alignment) == "6-%d" % (7 + add)


def test_format_positions_random(klib):
    rng = np.random.default_rng(20240611)
    for i in range(3000):
        n = int(rng.integers(0, 400))
        density = rng.choice([0.02, 0.3, 0.5, 0.9, 0.99])
        c = (rng.random(n) < density).tolist()
        wa = bool(i & 1)
        assert format_lib(klib, c, wa) == format_positions_ref(c, wa)


def test_format_positions_short_buffer(klib):
    c = [True, False] * 50 + [True] * 30
    want = format_positions_ref(c, False).encode()
    words = pack_bits(c)
    assert klib.kaamer_format_positions(words.ctypes.data, len(c), 0, None, 0) == len(want)
    for cap in (1, 2, 7, len(want) - 1, len(want)):
        raw = (C.c_char * (cap + 16))()
        C.memset(raw, 0x55, cap + 16)
        need = klib.kaamer_format_positions(words.ctypes.data, len(c), 0, C.cast(raw, C.c_char_p), cap)
        assert need == len(want)                       # the length needed, whatever the buffer holds
        got = bytes(raw)
        assert got[cap:] == b"\x55" * 16               # nothing past cap
        assert got[:cap - 1] == want[:cap - 1] and got[cap - 1] == 0
    # bits beyond n_bits in the last word are ignored
    w = np.array([0xFFFFFFFFFFFFFFFF], np.uint64)
    buf = C.create_string_buffer(32)
    klib.kaamer_format_positions(w.ctypes.data, 10, 0, buf, 32)
    assert buf.value == b"1-10"
