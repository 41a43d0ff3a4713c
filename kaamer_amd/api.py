"""Python plumbing over the C ABI: builds images from numpy buffers, opens an
index on a device, and runs batches either from host buffers or from
torch-owned device tensors (device memory and streams are torch's job here,
nothing else).  All compute happens inside libkaamer_hip.so.
"""
import ctypes as C
import os

import numpy as np

from . import abi


def pack_sequences(seqs):
    """list of bytes/str -> (uint8 array, uint64 offsets[n+1])"""
    bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in seqs]
    offs = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    buf = np.frombuffer(b"".join(bs), dtype=np.uint8).copy() if bs else np.zeros(0, np.uint8)
    return buf, offs


def packed_batch(seqs=None, packed=None):
    """seqs, or packed=(buf, offs) -> (buf u8, offs u64, (seqs pointer or None, offsets pointer, n_seqs)): the contiguous
    arrays, which the caller holds across the call, and the packed-batch arguments that point into them"""
    buf, offs = packed if packed is not None else pack_sequences(seqs)
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    return buf, offs, (buf.ctypes.data if len(buf) else None, offs.ctypes.data, len(offs) - 1)


def _proteins_args(seqs, packed, ids):
    """the builders' (seqs, offsets, ids, n_proteins) -> (what keeps the arrays alive, the four arguments)"""
    buf, offs, batch = packed_batch(seqs, packed)
    ids = np.ascontiguousarray(ids, dtype=np.uint32) if ids is not None else None
    return (buf, offs, ids), (buf.ctypes.data, batch[1], ids.ctypes.data if ids is not None else None, batch[2])


def _new(fn, *args):
    """fn(*args, &handle), checked -> the handle"""
    h = C.c_void_p()
    abi.check(fn(*args, C.byref(h)))
    return h


def _u64s(fn, n, *args):
    """fn(*args, out) with out a u64 array of n, checked -> the n values"""
    out = (C.c_uint64 * n)()
    abi.check(fn(*args, out))
    return [int(v) for v in out]


def _info(fn, handle, n, names):
    """an info getter of the library, which fills n u64 -> dict of the first len(names) of them"""
    return dict(zip(names, _u64s(fn, n, handle)))


class _Handle:
    """One object of the library behind `_h`: close() frees it through the function _FREE names, once, and __del__ closes
    what was not closed without ever raising."""
    _FREE = None

    def __init__(self, handle):
        self._h = handle if isinstance(handle, C.c_void_p) else C.c_void_p(handle)

    def _free(self, h):
        getattr(abi.lib(), self._FREE)(h)

    def close(self):
        h, self._h = self._h, None
        if h:
            self._free(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Image(_Handle):
    """Host copy of one shard's table (the builder's output)."""
    _FREE = "kaamer_image_free"

    @classmethod
    def from_pairs(cls, keys, ids, shard=0, n_shards=1, load_factor=0.5):
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        pairs = np.empty((len(keys), 2), dtype=np.uint32)
        pairs[:, 0] = keys
        pairs[:, 1] = ids
        return cls(_new(abi.lib().kaamer_image_build_pairs, pairs.ctypes.data, len(keys), shard, n_shards, load_factor))

    @classmethod
    def from_proteins(cls, seqs=None, ids=None, packed=None, shard=0, n_shards=1, load_factor=0.5, device=None):
        """device=None: the host builder; device=d: the same image built on GPU d (byte-identical)."""
        keep, proteins = _proteins_args(seqs, packed, ids)
        if device is None:
            return cls(_new(abi.lib().kaamer_image_build_proteins, *proteins, shard, n_shards, load_factor))
        return cls(_new(abi.lib().kaamer_image_build_proteins_device, *proteins, shard, n_shards, load_factor, int(device)))

    @classmethod
    def from_fasta_text(cls, text, shard=0, n_shards=1, load_factor=0.5, device=0):
        """(proteins, image) of a database FASTA text, read and built on GPU `device` (kaamer_image_build_fasta_device): the
        sequences stay there between the reader and the builder."""
        text = bytes(text)
        p, im = C.c_void_p(), C.c_void_p()
        abi.check(abi.lib().kaamer_image_build_fasta_device(text, len(text), shard, n_shards, load_factor, int(device), C.byref(p), C.byref(im)))
        return Proteins(p), cls(im)

    @classmethod
    def from_tsv_text(cls, text, shard=0, n_shards=1, load_factor=0.5, device=0):
        """(proteins, image) of a database TSV text (header line first), read and built on GPU `device`
        (kaamer_image_build_tsv_device): the sequences stay there between the reader and the builder."""
        text = bytes(text)
        p, im = C.c_void_p(), C.c_void_p()
        abi.check(abi.lib().kaamer_image_build_tsv_device(text, len(text), shard, n_shards, load_factor, int(device), C.byref(p), C.byref(im)))
        return Proteins(p), cls(im)

    @classmethod
    def from_embl_text(cls, text, shard=0, n_shards=1, load_factor=0.5, device=0):
        """(proteins, image) of a database EMBL text (UniProt flat file), read and built on GPU `device`
        (kaamer_image_build_embl_device): the indexed sequences stay there between the reader and the builder."""
        text = bytes(text)
        p, im = C.c_void_p(), C.c_void_p()
        abi.check(abi.lib().kaamer_image_build_embl_device(text, len(text), shard, n_shards, load_factor, int(device), C.byref(p), C.byref(im)))
        return Proteins(p), cls(im)

    @classmethod
    def from_gbk_text(cls, text, shard=0, n_shards=1, load_factor=0.5, device=0):
        """(proteins, image) of a database GBK text (GenBank / GenPept flat file), read and built on GPU `device`
        (kaamer_image_build_gbk_device): the sequences stay there between the reader and the builder."""
        text = bytes(text)
        p, im = C.c_void_p(), C.c_void_p()
        abi.check(abi.lib().kaamer_image_build_gbk_device(text, len(text), shard, n_shards, load_factor, int(device), C.byref(p), C.byref(im)))
        return Proteins(p), cls(im)

    @classmethod
    def merge(cls, images, load_factor=0.5, device=None):
        """kaamer-db -merge: the union of images of one shard (kaamer_image_merge).  device=None: on the host;
        device=d: the same image made on GPU d (byte-identical)."""
        images = list(images)
        arr = (C.c_void_p * max(1, len(images)))(*[im._h for im in images])
        if device is None:
            return cls(_new(abi.lib().kaamer_image_merge, arr, len(images), load_factor))
        return cls(_new(abi.lib().kaamer_image_merge_device, arr, len(images), load_factor, int(device)))

    @classmethod
    def load(cls, path):
        return cls(_new(abi.lib().kaamer_image_load, str(path).encode()))

    def save(self, path):
        abi.check(abi.lib().kaamer_image_save(self._h, str(path).encode()))

    @property
    def load_factor(self):
        return float(abi.lib().kaamer_image_load_factor(self._h))

    def stats(self):
        s = abi.ImageStats()
        abi.check(abi.lib().kaamer_image_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def get(self, key):
        n = abi.lib().kaamer_image_get(self._h, int(key), None, 0)
        out = np.zeros(n, dtype=np.uint32)
        if n:
            abi.lib().kaamer_image_get(self._h, int(key), out.ctypes.data, n)
        return out


class Proteins(_Handle):
    """What makedb accepts from a database file (ids, sequences, annotations): kaamer_makedb_fasta / _tsv
    (pkg/makedb/inputFASTA.go, inputTSV.go) and the table kaamer_fetch_hits reads (search.go:454-470)."""
    _FREE = "kaamer_proteins_free"

    @classmethod
    def _make(cls, fn, text):
        text = bytes(text)
        return cls(_new(fn, text, len(text)))

    @classmethod
    def from_fasta(cls, text, device=None, nb_before=0, more=False):
        """device=None: kaamer_makedb_fasta on the host.  device=d: the same table read on GPU d (kaamer_makedb_fasta_device);
        there `text` may be a piece cut at text_cut_fasta: nb_before = the '>' lines in front of it, more = another piece follows."""
        if device is None:
            if nb_before or more:
                raise ValueError("nb_before / more belong to the device reader")
            return cls._make(abi.lib().kaamer_makedb_fasta, text)
        text = bytes(text)
        return cls(_new(abi.lib().kaamer_makedb_fasta_device, text, len(text), int(nb_before), int(bool(more)), int(device)))

    @classmethod
    def from_tsv(cls, text, device=None, header=None, id_base=0):
        """device=None: kaamer_makedb_tsv on the host.  device=d: the same table read on GPU d (kaamer_makedb_tsv_device);
        there `text` may be a piece of a file cut at any line end: header = the file's header line without its line end (every
        line of the piece is a row then), id_base = the rows accepted in front of the piece (len() of the pieces before)."""
        if device is None:
            if header is not None or id_base:
                raise ValueError("header / id_base belong to the device reader")
            return cls._make(abi.lib().kaamer_makedb_tsv, text)
        text = bytes(text)
        header = None if header is None else bytes(header)
        return cls(_new(abi.lib().kaamer_makedb_tsv_device, text, len(text), header, len(header or b""), int(id_base), int(device)))

    @classmethod
    def from_embl(cls, text, device=None, nb_before=0):
        """device=None: kaamer_makedb_embl on the host.  device=d: the same table read on GPU d (kaamer_makedb_embl_device);
        there `text` may be a piece cut at text_cut_embl: nb_before = the "//" lines in front of it."""
        if device is None:
            if nb_before:
                raise ValueError("nb_before belongs to the device reader")
            return cls._make(abi.lib().kaamer_makedb_embl, text)
        text = bytes(text)
        return cls(_new(abi.lib().kaamer_makedb_embl_device, text, len(text), int(nb_before), int(device)))

    @classmethod
    def from_gbk(cls, text, device=None, nb_before=0):
        """device=None: kaamer_makedb_gbk on the host.  device=d: the same table read on GPU d (kaamer_makedb_gbk_device);
        there `text` may be a piece cut at text_cut_gbk: nb_before = the "//" lines in front of it."""
        if device is None:
            if nb_before:
                raise ValueError("nb_before belongs to the device reader")
            return cls._make(abi.lib().kaamer_makedb_gbk, text)
        text = bytes(text)
        return cls(_new(abi.lib().kaamer_makedb_gbk_device, text, len(text), int(nb_before), int(device)))

    @classmethod
    def from_text(cls, text, fmt, offset=0, length=None, strict_scanner=False):
        """kaamer_makedb_text_range: fmt is abi.FASTA / TSV / EMBL / GBK; offset / length are kaamer-db -make's -offset / -length
        (length=None: the flag's default, the rest of the file)."""
        text = bytes(text)
        return cls(_new(abi.lib().kaamer_makedb_text_range, text, len(text), int(fmt), int(bool(strict_scanner)), int(offset),
                        abi.MAKEDB_LENGTH_ALL if length is None else int(length)))

    @classmethod
    def merge(cls, tables):
        """kaamer-db -merge on the protein tables (kaamer_proteins_merge): records in argument order, a later record of an id wins"""
        tables = list(tables)
        arr = (C.c_void_p * max(1, len(tables)))(*[t._h for t in tables])
        return cls(_new(abi.lib().kaamer_proteins_merge, arr, len(tables)))

    @classmethod
    def load(cls, path):
        return cls(_new(abi.lib().kaamer_proteins_load, str(path).encode()))

    def save(self, path):
        abi.check(abi.lib().kaamer_proteins_save(self._h, str(path).encode()))

    def __len__(self):
        return abi.lib().kaamer_proteins_count(self._h)

    @property
    def ids(self):
        n = len(self)
        return np.ctypeslib.as_array(abi.lib().kaamer_proteins_ids(self._h), shape=(n,)).copy() if n else np.zeros(0, np.uint32)

    @property
    def packed(self):
        n = len(self)
        offs = np.ctypeslib.as_array(abi.lib().kaamer_proteins_offsets(self._h), shape=(n + 1,)).copy()
        buf = np.ctypeslib.as_array(abi.lib().kaamer_proteins_seqs(self._h), shape=(int(offs[-1]),)).copy() \
            if offs[-1] else np.zeros(0, np.uint8)
        return buf, offs

    @property
    def feature_names(self):
        L = abi.lib()
        return [L.kaamer_proteins_feature_name(self._h, i) for i in range(L.kaamer_proteins_n_features(self._h))]

    def stats(self):
        out = (C.c_uint64 * 3)()
        abi.lib().kaamer_proteins_stats(self._h, out)
        return dict(NumberOfProteins=out[0], NumberOfAA=out[1], NumberOfKmers=out[2], Features=self.feature_names)

    def image(self, shard=0, n_shards=1, load_factor=0.5, device=None):
        if device is None:
            return Image(_new(abi.lib().kaamer_image_build_makedb, self._h, shard, n_shards, load_factor))
        return Image(_new(abi.lib().kaamer_image_build_makedb_device, self._h, shard, n_shards, load_factor, int(device)))

    def fetch_hits(self, ids):
        """[None | dict(EntryId, Sequence, Length, Features)] per protein id (protein.proto)"""
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        ent = (abi.ProteinEntry * max(1, len(ids)))()
        abi.check(abi.lib().kaamer_fetch_hits(self._h, ids.ctypes.data, len(ids), ent))
        names = self.feature_names
        out = []
        for e in ent[:len(ids)]:
            if not e.found:
                out.append(None)
                continue
            fo = [e.feature_off[i] for i in range(e.n_features + 1)]
            blob = C.string_at(e.features + fo[0], fo[-1] - fo[0]) if fo[-1] > fo[0] else b""
            out.append(dict(EntryId=C.string_at(e.entry_id, e.entry_id_len), Sequence=C.string_at(e.sequence, e.sequence_len),
                            Length=e.length,
                            Features={names[i]: blob[fo[i] - fo[0]:fo[i + 1] - fo[0]] for i in range(e.n_features)}))
        return out


def build_image_from_proteins(seqs, ids=None, **kw):
    return Image.from_proteins(seqs, ids=ids, **kw)


META_DTYPE = np.dtype([("src_seq", "<u4"), ("size_in_kmer", "<i4"), ("start_position", "<i4"), ("end_position", "<i4"),
                       ("plus_strand", "<i4"), ("aa_len", "<u4"), ("aa_off", "<u8"), ("sa_off", "<u4"), ("sa_len", "<u4")])


SPAN_DTYPE = np.dtype([("name_off", "<u4"), ("name_len", "<u4"), ("seq_off", "<u4"), ("seq_len", "<u4")])   # kaamer_text_span


class TopResult:
    """Host view of one kaamer_batch_top (copied out, the C object is freed): the reported queries
    (`rep_query`, `meta`, `trim`, CSR `top_off` + `top_pid` / `top_kmatch` / `top_first_pos`, `orf_aa`),
    plus dense per-query views for convenience (`top_cnt[n_queries]`, `dense()`).  `text_spans`: one SPAN_DTYPE item
    per record of the text for a result of the text calls (kaamer_batch_top_text_spans), else None."""

    def __init__(self, out):
        o = out.contents
        n, r, k = o.n_queries, o.n_reported, o.max_results
        self.n_queries, self.n_reported, self.max_results = n, r, k
        z = np.zeros(0, np.uint32)
        self.rep_query = np.ctypeslib.as_array(o.rep_query, shape=(r,)).copy() if r else z
        meta = np.ctypeslib.as_array(C.cast(o.q, C.POINTER(C.c_uint8)), shape=(r * C.sizeof(abi.QueryMeta),)).copy() \
            if r else np.zeros(0, np.uint8)
        self.meta = meta.view(META_DTYPE)
        self.trim = np.ctypeslib.as_array(o.trim, shape=(r,)).copy() if r else np.zeros(0, np.int32)
        self.top_off = np.ctypeslib.as_array(o.top_off, shape=(r + 1,)).copy()
        ne = int(self.top_off[r])
        self.top_pid = np.ctypeslib.as_array(o.top_pid, shape=(ne,)).copy() if ne else z
        self.top_kmatch = np.ctypeslib.as_array(o.top_kmatch, shape=(ne,)).copy() if ne else z
        self.top_first_pos = np.ctypeslib.as_array(o.top_first_pos, shape=(ne,)).copy() if ne else z
        aa_len = int((self.meta["aa_off"] + self.meta["aa_len"]).max()) if r and bool(o.orf_aa) else 0
        self.orf_aa = np.ctypeslib.as_array(o.orf_aa, shape=(aa_len,)).copy() if aa_len else np.zeros(0, np.uint8)
        self.counters = o.counters.as_dict()
        self.top_cnt = np.zeros(n, np.uint32)
        if r:
            self.top_cnt[self.rep_query] = np.diff(self.top_off.astype(np.int64)).astype(np.uint32)
        # PositionHits of the reported hits (kaamer_batch_top_positions): None unless the call asked for them
        self.pos_bits_len = self.pos_off = self.pos_bits = None
        pl, po, pb = C.POINTER(C.c_int32)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)()
        abi.check(abi.lib().kaamer_batch_top_positions(out, C.byref(pl), C.byref(po), C.byref(pb)))
        if bool(po) and bool(pb):
            self.pos_bits_len = np.ctypeslib.as_array(pl, shape=(r,)).copy() if r else np.zeros(0, np.int32)
            self.pos_off = np.ctypeslib.as_array(po, shape=(ne + 1,)).copy()
            nw = int(self.pos_off[ne])
            self.pos_bits = np.ctypeslib.as_array(pb, shape=(nw,)).copy() if nw else np.zeros(0, np.uint64)
        # the alignments of the reported hits (kaamer_batch_top_alignments): None unless the call asked for them; else one
        # dict per CSR entry (fields of kaamer_alignment; "aln": the three rows, None for a result without text), and the
        # CSR arrays above are in the reference's final order (BitScore descending)
        self.text_spans = None
        sp, ns = C.POINTER(abi.TextSpan)(), C.c_uint32()
        abi.check(abi.lib().kaamer_batch_top_text_spans(out, C.byref(sp), C.byref(ns)))
        if bool(sp):
            self.text_spans = np.ctypeslib.as_array(C.cast(sp, C.POINTER(C.c_uint8)), shape=(ns.value * 16,)).copy().view(SPAN_DTYPE) \
                if ns.value else np.zeros(0, SPAN_DTYPE)
        # the text a BGZF call inflated on the device (kaamer_batch_top_text): what text_spans index; None for other calls
        self.text = None
        tp, tn = C.c_void_p(), C.c_uint64()
        abi.check(abi.lib().kaamer_batch_top_text(out, C.byref(tp), C.byref(tn)))
        if tp.value:
            self.text = C.string_at(tp.value, tn.value)
        # the TSV rows of a call with tsv=... (kaamer_batch_top_tsv): bytes, and the first byte of every row + the total; None
        # for other calls
        self.tsv = self.tsv_line_off = None
        if hasattr(abi.lib(), "kaamer_batch_top_tsv"):
            vp, vn, vo = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint64)()
            abi.check(abi.lib().kaamer_batch_top_tsv(out, C.byref(vp), C.byref(vn), C.byref(vo)))
            if bool(vo):
                self.tsv = C.string_at(vp.value, vn.value) if vn.value else b""
                self.tsv_line_off = np.ctypeslib.as_array(vo, shape=(ne + 1,)).copy()
        # the JSON objects of a call with json=... (kaamer_batch_top_json): bytes, and the '{' of every object + the total
        self.json = self.json_obj_off = None
        if hasattr(abi.lib(), "kaamer_batch_top_json"):
            vp, vn, vo = C.c_void_p(), C.c_uint64(), C.POINTER(C.c_uint64)()
            abi.check(abi.lib().kaamer_batch_top_json(out, C.byref(vp), C.byref(vn), C.byref(vo)))
            if bool(vo):
                self.json = C.string_at(vp.value, vn.value) if vn.value else b""
                self.json_obj_off = np.ctypeslib.as_array(vo, shape=(r + 1,)).copy()
        self.alignments = None
        items, text = C.POINTER(abi.Alignment)(), C.POINTER(C.c_char)()
        abi.check(abi.lib().kaamer_batch_top_alignments(out, C.byref(items), C.byref(text)))
        if bool(items):
            self.alignments = []
            for e in range(ne):
                a = items[e]
                d = {k: getattr(a, k) for k, _ in abi.Alignment._fields_ if k not in ("aln_off", "reserved")}
                d["aln"] = None
                if bool(text) and a.status == 0:
                    ln = a.length
                    raw = C.string_at(C.addressof(text.contents) + a.aln_off, 3 * ln) if ln else b""
                    d["aln"] = (raw[:ln].decode("latin-1"), raw[ln:2 * ln].decode("latin-1"), raw[2 * ln:].decode("latin-1"))
                self.alignments.append(d)

    def positions(self, i):
        """{protein id: bool[S]} of REPORTED query i (index into rep_query), shaped like BatchResult.positions: the
        PositionHits of its reported hits (search.go:442-452); S = pos_bits_len[i], the SizeInKmer as searched (for an
        ORF the untrimmed one, like top_first_pos)."""
        if self.pos_bits is None:
            raise ValueError("this result was not asked for positions (want_positions=True)")
        size = int(self.pos_bits_len[i])
        words = (size + 63) // 64
        out = {}
        for e in range(int(self.top_off[i]), int(self.top_off[i + 1])):
            w = self.pos_bits[int(self.pos_off[e]):int(self.pos_off[e]) + words]
            out[int(self.top_pid[e])] = np.unpackbits(w.view(np.uint8), bitorder="little")[:size].astype(bool)
        return out

    def dense(self):
        """(top_pid, top_kmatch) as [n_queries, max_results] arrays, zero beyond top_cnt"""
        pid = np.zeros((self.n_queries, self.max_results), np.uint32)
        km = np.zeros((self.n_queries, self.max_results), np.uint32)
        for i in range(self.n_reported):
            a, b = int(self.top_off[i]), int(self.top_off[i + 1])
            pid[self.rep_query[i], :b - a] = self.top_pid[a:b]
            km[self.rep_query[i], :b - a] = self.top_kmatch[a:b]
        return pid, km


class _BatchOwner:
    """frees one kaamer_batch_out when the last array that views its buffers is gone"""

    def __init__(self, out):
        self.out = out

    def __del__(self):
        try:
            if self.out is not None:
                abi.lib().kaamer_batch_free(self.out)
                self.out = None
        except Exception:
            pass


def _owned_view(owner, ptr, n, dtype):
    """numpy view of n items at `ptr` (a ctypes pointer) that keeps `owner` alive: the exporting ctypes array holds a
    reference to it, and every array derived from the view holds the exporter"""
    dtype = np.dtype(dtype)
    if n == 0:
        return np.zeros(0, dtype)
    raw = (C.c_uint8 * (n * dtype.itemsize)).from_address(C.cast(ptr, C.c_void_p).value)
    raw._owner = owner
    return np.frombuffer(raw, dtype=dtype)


class BatchResult:
    """Host view of one kaamer_batch_out: the arrays are views of the C object's buffers (no copies).  The buffers
    live as long as any of the arrays (or anything sliced from them) does: `ix.search(...).hit_pid` stays valid after
    the BatchResult itself is gone."""

    def __init__(self, out):
        o = out.contents
        own = _BatchOwner(out)
        n = o.n_queries
        self.n_queries = n
        self.meta = _owned_view(own, o.q, n, META_DTYPE)
        self.hit_off = _owned_view(own, o.hit_off, n + 1, np.uint64)
        self.hit_cnt = _owned_view(own, o.hit_cnt, n, np.uint32)
        nh = int(self.hit_off[n])
        self.hit_pid = _owned_view(own, o.hit_pid, nh, np.uint32)
        self.hit_kmatch = _owned_view(own, o.hit_kmatch, nh, np.uint32)
        self.hit_first_pos = _owned_view(own, o.hit_first_pos, nh, np.uint32)
        self.counters = o.counters.as_dict()
        self.pos_off = self.pos_bits = None
        if bool(o.pos_off) and bool(o.pos_bits):
            self.pos_off = _owned_view(own, o.pos_off, nh, np.uint64)
            nw = 0
            if nh:  # words in use = end of the last bitmap
                has = self.hit_cnt > 0
                last = (self.hit_off[:n][has] + self.hit_cnt[has].astype(np.uint64) - np.uint64(1)).astype(np.int64)
                words = (self.meta["size_in_kmer"][has].astype(np.int64) + 63) // 64
                nw = int((self.pos_off[last].astype(np.int64) + words).max())
            self.pos_bits = _owned_view(own, o.pos_bits, nw, np.uint64)
        aa_len = int((self.meta["aa_off"] + self.meta["aa_len"]).max()) if n and bool(o.orf_aa) else 0
        self.orf_aa = _owned_view(own, o.orf_aa, aa_len, np.uint8)
        sa_len = int((self.meta["sa_off"] + self.meta["sa_len"]).max()) if n and bool(o.starts_alt) else 0
        self.starts_alt = _owned_view(own, o.starts_alt, sa_len, np.int32)

    def close(self):
        """drops this object's views (the buffers go when no other array views them)"""
        for k in ("meta", "hit_off", "hit_cnt", "hit_pid", "hit_kmatch", "hit_first_pos", "pos_off", "pos_bits", "orf_aa", "starts_alt"):
            setattr(self, k, None)

    def span(self, q):
        """[first, last+1) of query q's hits in the hit arrays"""
        a = int(self.hit_off[q])
        return a, a + int(self.hit_cnt[q])

    def positions(self, q):
        """{protein id: bool[SizeInKmer]} of query q (PositionHits, search.go:442-452)."""
        a, b = self.span(q)
        size = int(self.meta["size_in_kmer"][q])
        out = {}
        words = (size + 63) // 64
        for i in range(a, b):
            w = self.pos_bits[int(self.pos_off[i]):int(self.pos_off[i]) + words]
            bits = np.unpackbits(w.view(np.uint8), bitorder="little")[:size].astype(bool)
            out[int(self.hit_pid[i])] = bits
        return out

    def hits(self, q):
        """{protein id: Kmatch} of query q (the parity object: SURVEY §2.1)."""
        a, b = self.span(q)
        return dict(zip(self.hit_pid[a:b].tolist(), self.hit_kmatch[a:b].tolist()))

    def first_pos(self, q):
        a, b = self.span(q)
        return dict(zip(self.hit_pid[a:b].tolist(), self.hit_first_pos[a:b].tolist()))


def _take_top(out):
    """a kaamer_batch_top the caller owns -> its TopResult (copied out); the C object is freed"""
    try:
        return TopResult(out)
    finally:
        abi.lib().kaamer_batch_top_free(out)


def _batch_call(ix, wait, seqs, packed, seq_type, want_positions, flat=True):
    """kaamer_[sharded_]{search,submit}_batch[_flat]: the full hit lists of a packed batch on an Index or a ShardedIndex.
    wait: search (-> BatchResult), else submit (-> FullTicket)"""
    buf, offs, batch = packed_batch(seqs, packed)
    stem = "kaamer_%s%s_batch" % (ix._PREFIX, "search" if wait else "submit")
    out = C.POINTER(abi.BatchOut)() if wait else C.c_void_p()
    if flat:
        abi.check(getattr(abi.lib(), stem + "_flat")(ix._h, *batch, seq_type, int(want_positions), C.byref(out)))
    else:
        bi = abi.BatchIn(*batch, seq_type, int(want_positions))
        abi.check(getattr(abi.lib(), stem)(ix._h, C.byref(bi), C.byref(out)))
    return BatchResult(out) if wait else FullTicket(out, sharded=bool(ix._PREFIX))


def _batch_top_call(ix, wait, seqs, packed, seq_type, top, want_positions, align, flat=True):
    """kaamer_[sharded_]{search,submit}_batch_top[_aln_flat|_pos_flat|_flat]: the reported hits of a packed batch on an Index
    or a ShardedIndex.  top: (min_k_ratio, min_k_match, max_results); the form is `align`'s, else want_positions', else the
    flat or the struct one.  wait: search (-> TopResult), else submit (-> TopTicket)"""
    buf, offs, batch = packed_batch(seqs, packed)
    stem = "kaamer_%s%s_batch_top" % (ix._PREFIX, "search" if wait else "submit")
    out = C.POINTER(abi.BatchTop)() if wait else C.c_void_p()
    if align is not None:
        abi.check(getattr(abi.lib(), stem + "_aln_flat")(ix._h, *batch, seq_type, *top, int(bool(want_positions)), *_align_args(align),
                                                         C.byref(out)))
    elif want_positions or flat:
        abi.check(getattr(abi.lib(), stem + ("_pos_flat" if want_positions else "_flat"))(ix._h, *batch, seq_type, *top, C.byref(out)))
    else:
        bi = abi.BatchIn(*batch, seq_type, 0)
        to = abi.TopnOpts(*top, 0, None, None, 0, 0)
        abi.check(getattr(abi.lib(), stem)(ix._h, C.byref(bi), C.byref(to), C.byref(out)))
    return _take_top(out) if wait else TopTicket(out, sharded=bool(ix._PREFIX))


class Index(_Handle):
    """The table resident in one device's HBM."""
    _FREE, _PREFIX, _STREAM = "kaamer_index_close", "", "stream"

    def __init__(self, handle, device):
        super().__init__(handle)
        self.device = device
        self.proteins = None   # attach_proteins

    @classmethod
    def from_image(cls, image, device=0):
        return cls(_new(abi.lib().kaamer_index_open_image, image._h, device), device)

    @classmethod
    def from_proteins(cls, seqs=None, ids=None, packed=None, shard=0, n_shards=1, load_factor=0.5, device=0):
        """The table built on the device it is searched on (kaamer_index_build_proteins): no image in between."""
        keep, proteins = _proteins_args(seqs, packed, ids)
        return cls(_new(abi.lib().kaamer_index_build_proteins, *proteins, shard, n_shards, load_factor, int(device)), device)

    @classmethod
    def from_fasta_text(cls, text, shard=0, n_shards=1, load_factor=0.5, device=0):
        """(proteins, index) of a database FASTA text, read and built on the device it is searched on (kaamer_index_build_fasta)"""
        text = bytes(text)
        p, ix = C.c_void_p(), C.c_void_p()
        abi.check(abi.lib().kaamer_index_build_fasta(text, len(text), shard, n_shards, load_factor, int(device), C.byref(p), C.byref(ix)))
        return Proteins(p), cls(ix, device)

    @classmethod
    def from_tsv_text(cls, text, shard=0, n_shards=1, load_factor=0.5, device=0):
        """(proteins, index) of a database TSV text (header line first), read and built on the device it is searched on
        (kaamer_index_build_tsv)"""
        text = bytes(text)
        p, ix = C.c_void_p(), C.c_void_p()
        abi.check(abi.lib().kaamer_index_build_tsv(text, len(text), shard, n_shards, load_factor, int(device), C.byref(p), C.byref(ix)))
        return Proteins(p), cls(ix, device)

    @classmethod
    def from_embl_text(cls, text, shard=0, n_shards=1, load_factor=0.5, device=0):
        """(proteins, index) of a database EMBL text, read and built on the device it is searched on (kaamer_index_build_embl)"""
        text = bytes(text)
        p, ix = C.c_void_p(), C.c_void_p()
        abi.check(abi.lib().kaamer_index_build_embl(text, len(text), shard, n_shards, load_factor, int(device), C.byref(p), C.byref(ix)))
        return Proteins(p), cls(ix, device)

    @classmethod
    def from_gbk_text(cls, text, shard=0, n_shards=1, load_factor=0.5, device=0):
        """(proteins, index) of a database GBK text, read and built on the device it is searched on (kaamer_index_build_gbk)"""
        text = bytes(text)
        p, ix = C.c_void_p(), C.c_void_p()
        abi.check(abi.lib().kaamer_index_build_gbk(text, len(text), shard, n_shards, load_factor, int(device), C.byref(p), C.byref(ix)))
        return Proteins(p), cls(ix, device)

    @classmethod
    def open(cls, path, device=0):
        return cls(_new(abi.lib().kaamer_index_open, str(path).encode(), device), device)

    def stats(self):
        s = abi.ImageStats()
        abi.check(abi.lib().kaamer_index_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def search(self, seqs=None, packed=None, seq_type=abi.PROTEIN, want_positions=False, flat=True):
        """Host-buffer form (kaamer_search_batch_flat: the entry point a cgo shim binds; flat=False: the struct form
        kaamer_search_batch)."""
        return _batch_call(self, True, seqs, packed, seq_type, want_positions, flat)

    def submit(self, seqs=None, packed=None, seq_type=abi.PROTEIN, want_positions=False):
        """kaamer_submit_batch_flat -> a ticket whose wait() returns the BatchResult (full hit lists)"""
        return _batch_call(self, False, seqs, packed, seq_type, want_positions)

    def search_top(self, seqs=None, packed=None, seq_type=abi.PROTEIN, min_k_ratio=0.05, min_k_match=10, max_results=10, flat=True,
                   want_positions=False, align=None):
        """Host-buffer form that returns the reported hits only (kaamer_search_batch_top_flat; flat=False: the struct
        form): sortMapByValue order, SetBestStartCodon for nucleotide/reads, FilterResults -- all on the device.
        want_positions: the PositionHits bitmaps of the reported hits come along (kaamer_search_batch_top_pos_flat;
        TopResult.positions).
        align: dict(sub_matrix="blosum62", gap_open=11, gap_extend=1, text=True) -- every reported hit aligned with its
        query in the same call (kaamer_search_batch_top_aln_flat; needs attach_proteins): TopResult.alignments, hits in
        BitScore order."""
        return _batch_top_call(self, True, seqs, packed, seq_type, (min_k_ratio, min_k_match, max_results), want_positions, align, flat)

    def submit_top(self, seqs=None, packed=None, seq_type=abi.PROTEIN, min_k_ratio=0.05, min_k_match=10, max_results=10, flat=True,
                   want_positions=False, align=None):
        """kaamer_submit_batch_top[_flat]: the batch is copied and enqueued on a free slot; -> a ticket whose wait() returns
        the TopResult.  Several tickets may be in flight; submit blocks while every slot is busy.
        want_positions: kaamer_submit_batch_top_pos_flat (the bitmaps of the reported hits come along).
        align: as search_top's -- kaamer_submit_batch_top_aln_flat: the reported hits aligned with their queries in the
        same call (needs attach_proteins); the ticket's TopResult carries `alignments`, hits in BitScore order."""
        return _batch_top_call(self, False, seqs, packed, seq_type, (min_k_ratio, min_k_match, max_results), want_positions, align, flat)

    def _text_call(self, kind, data, extra, top, tsv, wait, align=None, json=None):
        """kaamer_{search,submit}_{kind}_top[_tsv|_aln_tsv]_flat -- kind: text, fasta or bgzf; extra: the kind's arguments
        between the data and the sequence type, and the sequence type; top: (min_k_ratio, min_k_match, max_results); wait:
        search (-> TopResult), else submit (-> TopTicket)"""
        data = data.encode("latin-1") if isinstance(data, str) else bytes(data)
        if align is not None and tsv is None:
            raise ValueError("align=... on a text call comes with tsv=...: the call returns the -aln rows")
        if json is not None and (tsv is not None or align is not None):
            raise ValueError("json=... comes alone: one response format per call, and -aln JSON is not written")
        form = "_json" if json is not None else "" if tsv is None else "_tsv" if align is None else "_aln_tsv"
        fn = getattr(abi.lib(), "kaamer_%s_%s_top%s_flat" % ("search" if wait else "submit", kind, form))
        out = C.POINTER(abi.BatchTop)() if wait else C.c_void_p()
        more = (_tsv_args(tsv) if tsv is not None else ()) + (_align_args(align)[:3] if align is not None else ())
        if json is not None:
            more = (int(bool(json.get("positions"))),)
        abi.check(fn(self._h, data, len(data), *extra, *top, *more, C.byref(out)))
        return _take_top(out) if wait else TopTicket(out)

    def search_text_top(self, text, seq_type=abi.READS, min_k_ratio=0.05, min_k_match=10, max_results=10, fmt="fastq", tsv=None, align=None, json=None):
        """kaamer_search_text_top_flat: FASTQ text (bytes) in, the reported hits out -- the text is parsed on the device
        (GetQueriesFastq) and searched as search_top searches the packed batch.  TopResult.text_spans: name and sequence of
        every record as offsets into `text`; rep_query / meta["src_seq"] index the records.
        tsv=dict(positions=..., annotations=...): kaamer_search_text_top_tsv_flat -- the TSV rows of the reported hits are
        written on the device too (needs attach_subject_text): TopResult.tsv, .tsv_line_off.
        align=dict(sub_matrix=..., gap_open=..., gap_extend=...) with tsv: kaamer_search_text_top_aln_tsv_flat -- the reported
        hits are aligned in between (needs attach_proteins too) and the rows are the -aln form; TopResult.alignments carries
        the numbers (no text), the hits are in BitScore order.
        json=dict(positions=...): kaamer_search_text_top_json_flat -- the JSON objects of the reported queries are written on
        the device too (needs attach_subject_json): TopResult.json, .json_obj_off; positions matters for PROTEIN only."""
        return self._text_call("text", text, (1 if fmt == "fastq" else 0, seq_type), (min_k_ratio, min_k_match, max_results), tsv, True, align, json)

    def search_bgzf_top(self, data, seq_type=abi.READS, min_k_ratio=0.05, min_k_match=10, max_results=10, tsv=None, align=None, json=None):
        """kaamer_search_bgzf_top_flat: whole BGZF blocks of FASTQ (bytes) in, the reported hits out -- the compressed bytes
        are uploaded, inflated, parsed and searched on the device.  TopResult.text: the inflated text; text_spans index it.
        Bytes that are not whole BGZF blocks: KaamerError E_ARG; a block that does not inflate: E_FORMAT.
        tsv, align: as search_text_top's (kaamer_search_bgzf_top_tsv_flat / _aln_tsv_flat)."""
        return self._text_call("bgzf", bytes(data), (seq_type,), (min_k_ratio, min_k_match, max_results), tsv, True, align, json)

    def submit_bgzf_top(self, data, seq_type=abi.READS, min_k_ratio=0.05, min_k_match=10, max_results=10, tsv=None, align=None, json=None):
        """kaamer_submit_bgzf_top_flat -> a ticket whose wait() returns the TopResult (with text and text_spans); tsv, align:
        as search_text_top's"""
        return self._text_call("bgzf", bytes(data), (seq_type,), (min_k_ratio, min_k_match, max_results), tsv, False, align, json)

    def submit_text_top(self, text, seq_type=abi.READS, min_k_ratio=0.05, min_k_match=10, max_results=10, fmt="fastq", tsv=None, align=None, json=None):
        """kaamer_submit_text_top_flat -> a ticket whose wait() returns the TopResult (with text_spans); tsv, align: as
        search_text_top's"""
        return self._text_call("text", text, (1 if fmt == "fastq" else 0, seq_type), (min_k_ratio, min_k_match, max_results), tsv, False, align, json)

    def search_fasta_top(self, text, seq_type=abi.PROTEIN, upper_last=False, min_k_ratio=0.05, min_k_match=10, max_results=10, tsv=None, align=None, json=None):
        """kaamer_search_fasta_top_flat: FASTA text (bytes) in, the reported hits out -- the text is parsed on the device
        (GetQueriesFasta) and searched as search_top searches the packed batch.  seq_type: PROTEIN, NUCLEOTIDE or READS
        (with a genetic code).  upper_last: more input follows this text, its last record is upper-cased too.
        TopResult.text_spans: name and sequence range of every record as offsets into `text`.
        tsv, align: as search_text_top's (kaamer_search_fasta_top_tsv_flat / _aln_tsv_flat)."""
        return self._text_call("fasta", text, (seq_type, int(bool(upper_last))), (min_k_ratio, min_k_match, max_results), tsv, True, align, json)

    def submit_fasta_top(self, text, seq_type=abi.PROTEIN, upper_last=False, min_k_ratio=0.05, min_k_match=10, max_results=10, tsv=None, align=None, json=None):
        """kaamer_submit_fasta_top_flat -> a ticket whose wait() returns the TopResult (with text_spans); tsv, align: as
        search_text_top's"""
        return self._text_call("fasta", text, (seq_type, int(bool(upper_last))), (min_k_ratio, min_k_match, max_results), tsv, False, align, json)

    def tsv_aln_info(self):
        """kaamer_index_tsv_aln_info -> dict(host_batches: batches of the align + tsv text calls whose rows the host printed,
        raw_count: raw scores the stages' table holds)"""
        return _info(abi.lib().kaamer_index_tsv_aln_info, self._h, 2, ("host_batches", "raw_count"))

    def set_tsv_aln_raw_count(self, n):
        """kaamer_index_set_tsv_aln_raw_count (a test entry): the stages' table holds the first n raw scores only; 0: all"""
        abi.check(abi.lib().kaamer_index_set_tsv_aln_raw_count(self._h, int(n)))

    def stream(self, seq_type=abi.READS, min_k_ratio=0.05, min_k_match=10, max_results=10, want_positions=False, align=None):
        """kaamer_stream_open[_pos|_aln]_flat; align: as search_top's (needs attach_proteins)"""
        return TopStream(self, seq_type, min_k_ratio, min_k_match, max_results, want_positions, align)

    def attach_proteins(self, proteins):
        """kaamer_index_attach_proteins: the table's Protein.Sequence entries become resident next to the index (the
        subjects of search_top(align=...)).  The table is borrowed by the library: the index keeps it alive."""
        abi.check(abi.lib().kaamer_index_attach_proteins(self._h, proteins._h))
        self.proteins = proteins

    def attach_subject_text(self, proteins):
        """kaamer_index_attach_subject_text: EntryId, Length and the annotation columns of every entry become resident
        next to the index: what the TSV rows print of a hit (search_*_top(tsv=...), TsvStage)."""
        abi.check(abi.lib().kaamer_index_attach_subject_text(self._h, proteins._h))

    def attach_subject_json(self, proteins):
        """kaamer_index_attach_subject_json: every entry's HitEntries value (the Protein object as JSON) becomes resident
        next to the index; what the calls that return JSON objects read"""
        abi.check(abi.lib().kaamer_index_attach_subject_json(self._h, proteins._h))

    def subject_json_info(self):
        """kaamer_index_subject_json_info -> dict(table_bytes, entries, max_entry)"""
        return _info(abi.lib().kaamer_index_subject_json_info, self._h, 4, ("table_bytes", "entries", "max_entry"))

    def subject_text_info(self):
        """kaamer_index_subject_text_info -> dict"""
        return _info(abi.lib().kaamer_index_subject_text_info, self._h, 4, ("table_bytes", "entries", "max_row_suffix", "features"))

    def set_json_bounds(self, nbytes, objects):
        """kaamer_index_set_json_bounds: the first bounds (bytes, objects) of the json=... calls on every slot; 0: the rule"""
        abi.check(abi.lib().kaamer_index_set_json_bounds(self._h, int(nbytes), int(objects)))

    def set_tsv_bounds(self, nbytes, lines):
        """kaamer_index_set_tsv_bounds: the first bounds (bytes, rows) of the tsv=... calls on every slot; 0: the rule"""
        abi.check(abi.lib().kaamer_index_set_tsv_bounds(self._h, int(nbytes), int(lines)))

    def align_info(self):
        """kaamer_index_align_info -> dict"""
        return _info(abi.lib().kaamer_index_align_info, self._h, 8,
                     ("table_bytes", "entries", "max_subject_len", "number_of_aa", "budget_bytes", "waves", "slab_bytes", "long_waves"))

    def set_align_budget(self, nbytes):
        """kaamer_index_set_align_budget: bytes of direction array one call's alignment stage may hold; 0: the default"""
        abi.check(abi.lib().kaamer_index_set_align_budget(self._h, int(nbytes)))

    def set_top_positions_bound(self, words):
        """kaamer_index_set_top_positions_bound: the first bitmap bound (u64 words) of the want_positions calls; 0: the rule"""
        abi.check(abi.lib().kaamer_index_set_top_positions_bound(self._h, int(words)))


class ShardedIndex(_Handle):
    """kaamer_index_open_sharded*: one handle over W hash-prefix shards, each resident on its own device, driven from
    one process (no communicator)."""
    _FREE, _PREFIX, _STREAM = "kaamer_sharded_index_close", "sharded_", "sharded_stream"

    def __init__(self, handle):
        super().__init__(handle)
        self.proteins = None   # attach_proteins

    @classmethod
    def from_images(cls, images, devices):
        n = len(images)
        arr = (C.c_void_p * n)(*[im._h for im in images])
        return cls(_new(abi.lib().kaamer_index_open_sharded_images, arr, (C.c_int * n)(*devices), n))

    @classmethod
    def open(cls, paths, devices):
        n = len(paths)
        arr = (C.c_char_p * n)(*[str(p).encode() for p in paths])
        return cls(_new(abi.lib().kaamer_index_open_sharded, arr, (C.c_int * n)(*devices), n))

    def search_top(self, seqs=None, packed=None, seq_type=abi.PROTEIN, min_k_ratio=0.05, min_k_match=10, max_results=10, flat=True,
                   want_positions=False, align=None):
        """What Index.search_top returns on an unsharded index of the whole database.  want_positions: the PositionHits
        bitmaps of the reported hits come along (kaamer_sharded_search_batch_top_pos_flat; TopResult.positions).
        align: as Index.search_top's -- every reported hit aligned with its query in the same call
        (kaamer_sharded_search_batch_top_aln_flat; needs attach_proteins): TopResult.alignments, hits in BitScore order."""
        return _batch_top_call(self, True, seqs, packed, seq_type, (min_k_ratio, min_k_match, max_results), want_positions, align, flat)

    def submit_top(self, seqs=None, packed=None, seq_type=abi.PROTEIN, min_k_ratio=0.05, min_k_match=10, max_results=10,
                   want_positions=False, align=None):
        """kaamer_sharded_submit_batch_top_flat -> a ticket (wait() -> TopResult); up to three calls in flight per handle.
        want_positions: kaamer_sharded_submit_batch_top_pos_flat (the bitmaps of the reported hits come along).
        align: as search_top's (kaamer_sharded_submit_batch_top_aln_flat)."""
        return _batch_top_call(self, False, seqs, packed, seq_type, (min_k_ratio, min_k_match, max_results), want_positions, align)

    def attach_proteins(self, proteins):
        """kaamer_sharded_index_attach_proteins: the table's Protein.Sequence entries become resident on the handle's
        devices, partitioned by id mod W (the subjects of search_top(align=...)).  The table is borrowed by the library:
        the handle keeps it alive."""
        abi.check(abi.lib().kaamer_sharded_index_attach_proteins(self._h, proteins._h))
        self.proteins = proteins

    def align_info(self):
        """kaamer_sharded_align_info -> dict"""
        return _info(abi.lib().kaamer_sharded_align_info, self._h, 8,
                     ("table_bytes", "largest_share", "entries", "max_subject_len", "number_of_aa", "segment_bytes", "need_bytes", "attempts"))

    def set_align_timing(self, on=True):
        """kaamer_sharded_index_set_align_timing: HIP events around the gather, assemble and alignment stages of later calls"""
        abi.check(abi.lib().kaamer_sharded_index_set_align_timing(self._h, int(bool(on))))

    def align_stage_info(self):
        """kaamer_sharded_align_stage_info -> dict (stage times in microseconds: zeros unless set_align_timing)"""
        return _info(abi.lib().kaamer_sharded_align_stage_info, self._h, 8,
                     ("timing", "gather_us", "assemble_us", "align_us", "ids_block_bytes", "waves", "slab_bytes", "long_waves"))

    def set_align_budget(self, nbytes):
        """kaamer_sharded_index_set_align_budget: bytes of direction array each owner's alignment stage may hold; 0: the default"""
        abi.check(abi.lib().kaamer_sharded_index_set_align_budget(self._h, int(nbytes)))

    def positions_info(self):
        """-> dict(ids_block_bytes, segment_bytes, need_words, attempts) of the last finished call with positions on the
        handle's first set (kaamer_sharded_positions_info)"""
        return _info(abi.lib().kaamer_sharded_positions_info, self._h, 4, ("ids_block_bytes", "segment_bytes", "need_words", "attempts"))

    def search(self, seqs=None, packed=None, seq_type=abi.PROTEIN, want_positions=False, flat=True):
        """The full hit lists (PositionHits bitmaps with want_positions): what Index.search returns on an unsharded index
        of the whole database (kaamer_sharded_search_batch_flat; flat=False: the struct form)."""
        return _batch_call(self, True, seqs, packed, seq_type, want_positions, flat)

    def submit(self, seqs=None, packed=None, seq_type=abi.PROTEIN, want_positions=False):
        """kaamer_sharded_submit_batch_flat -> a ticket whose wait() returns the BatchResult (full hit lists)"""
        return _batch_call(self, False, seqs, packed, seq_type, want_positions)

    def stream(self, seq_type=abi.READS, min_k_ratio=0.05, min_k_match=10, max_results=10, want_positions=False, align=None):
        """kaamer_sharded_stream_open[_pos|_aln]_flat: a FIFO of at most abi.SHARDED_SETS chunks on the handle"""
        return TopStream(self, seq_type, min_k_ratio, min_k_match, max_results, want_positions, align)

    def search_file(self, path, fmt="fastq", seq_type=abi.READS, min_k_ratio=0.05, min_k_match=10, max_results=10,
                    chunk_seqs=1 << 20, chunk_bytes=1 << 28, in_flight=0, strict=False, on_chunk=None, want_positions=False, align=None):
        """kaamer_sharded_search_file: Replicas.search_file on the sharded handle (in_flight: chunks per handle)"""
        return _search_file(self, path, fmt, seq_type, (min_k_ratio, min_k_match, max_results), chunk_seqs, chunk_bytes, in_flight, strict,
                            on_chunk, want_positions, align)

    def exchange_info(self):
        """-> dict(block_bytes, need_entries, queries, adaptive) of the last finished call on the handle's first set"""
        info = _info(abi.lib().kaamer_sharded_exchange_info, self._h, 4, ("block_bytes", "need_entries", "queries", "adaptive"))
        info["adaptive"] = bool(info["adaptive"])
        return info


class Replicas(_Handle):
    """kaamer_index_open_replicas*: the same database resident on several devices of ONE process; chunks of a read set are
    dealt round-robin (kaamer_replica_stream_*), or a whole file is searched (kaamer_search_file)."""
    _FREE, _STREAM = "kaamer_replicas_close", "replica_stream"

    CHUNK_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(abi.BatchTop))

    def __init__(self, handle):
        super().__init__(handle)
        self.proteins = None   # attach_proteins

    @classmethod
    def from_image(cls, image, devices):
        return cls(_new(abi.lib().kaamer_index_open_replicas_image, image._h, (C.c_int * len(devices))(*devices), len(devices)))

    @classmethod
    def open(cls, path, devices):
        return cls(_new(abi.lib().kaamer_index_open_replicas, str(path).encode(), (C.c_int * len(devices))(*devices), len(devices)))

    def __len__(self):
        return int(abi.lib().kaamer_replicas_count(self._h))

    def attach_proteins(self, proteins):
        """kaamer_replicas_attach_proteins: Index.attach_proteins on every replica (the subjects of search_file(align=...)
        and stream(align=...)).  The table is borrowed by the library: the set keeps it alive."""
        abi.check(abi.lib().kaamer_replicas_attach_proteins(self._h, proteins._h))
        self.proteins = proteins

    def stream(self, seq_type=abi.READS, min_k_ratio=0.05, min_k_match=10, max_results=10, want_positions=False, align=None):
        """kaamer_replica_stream_open[_pos|_aln]_flat: chunk k goes to replica k mod n, pop returns them in push order"""
        return TopStream(self, seq_type, min_k_ratio, min_k_match, max_results, want_positions, align)

    def search_file(self, path, fmt="fastq", seq_type=abi.READS, min_k_ratio=0.05, min_k_match=10, max_results=10,
                    chunk_seqs=1 << 20, chunk_bytes=1 << 28, in_flight=0, strict=False, on_chunk=None, want_positions=False, align=None):
        """kaamer_search_file.  on_chunk(first_seq, reads_handle, TopResult) per chunk, in input order (the reads handle is
        valid during the call: kaamer_reads_* accessors / api._reads_to_arrays).  -> summed counters
        want_positions / align (as Index.search_top's; align needs attach_proteins): kaamer_search_file_opts -- the
        TopResult of every chunk carries the bitmaps / the alignments of its reported hits."""
        return _search_file(self, path, fmt, seq_type, (min_k_ratio, min_k_match, max_results), chunk_seqs, chunk_bytes, in_flight, strict,
                            on_chunk, want_positions, align)

    TEXT_CHUNK_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(abi.BatchTop))

    @staticmethod
    def _text_chunk(first, text, length, spans, n_records, top):
        """what a kaamer_text_chunk_cb receives behind `user` -> on_chunk's (first_seq, text bytes, TopResult)"""
        return int(first), C.string_at(text, length), TopResult(top)

    def search_text_file(self, path, fmt="fastq", seq_type=abi.READS, min_k_ratio=0.05, min_k_match=10, max_results=10,
                         chunk_text_bytes=1 << 28, in_flight=0, on_chunk=None, device_inflate=False):
        """kaamer_search_text_file: the file's FASTQ text (plain or gzip) is cut into chunks of about chunk_text_bytes, each
        parsed and searched on a replica.  on_chunk(first_seq, text bytes, TopResult) per chunk, in input order; the
        TopResult's text_spans index `text`, its rep_query counts from the chunk's first record.  -> summed counters
        device_inflate (kaamer_search_text_file_opts): a BGZF file is inflated on the device, block by block; anything else
        in a gzip file falls back to the host inflater from that chunk on.  The concatenated texts are the same."""
        args = (self._h, str(path).encode(), 1 if fmt == "fastq" else 0, seq_type, min_k_ratio, min_k_match, max_results, int(chunk_text_bytes), in_flight)
        if device_inflate:
            return _drive_file(abi.lib().kaamer_search_text_file_opts, args + (1,), Replicas.TEXT_CHUNK_CB, Replicas._text_chunk, on_chunk)
        return _drive_file(abi.lib().kaamer_search_text_file, args, Replicas.TEXT_CHUNK_CB, Replicas._text_chunk, on_chunk)

    def search_fasta_file(self, path, seq_type=abi.PROTEIN, min_k_ratio=0.05, min_k_match=10, max_results=10, chunk_text_bytes=1 << 28,
                          in_flight=0, on_chunk=None):
        """kaamer_search_fasta_file: the file's FASTA text (plain or gzip) is cut into chunks of about chunk_text_bytes at
        kaamer_text_cut_fasta, each parsed and searched on a replica (every chunk but the last with upper_last).
        on_chunk(first_seq, text bytes, TopResult) per chunk, in input order, as search_text_file's.  -> summed counters"""
        args = (self._h, str(path).encode(), seq_type, min_k_ratio, min_k_match, max_results, int(chunk_text_bytes), in_flight)
        return _drive_file(abi.lib().kaamer_search_fasta_file, args, Replicas.TEXT_CHUNK_CB, Replicas._text_chunk, on_chunk)


def _tsv_args(tsv):
    """tsv=dict(positions=..., annotations=...) -> (extract_positions, annotations)"""
    return int(bool(tsv.get("positions"))), int(bool(tsv.get("annotations")))


def format_tsv_header(positions=False, annotations=False, proteins=None, align=False):
    """kaamer_format_tsv_header, or with align kaamer_format_tsv_aln_header: the header line of the TSV response
    (search.go:645-660) -> bytes"""
    fn = abi.lib().kaamer_format_tsv_aln_header if align else abi.lib().kaamer_format_tsv_header
    return _sized(fn, int(bool(positions)), int(bool(annotations)), proteins._h if proteins is not None else None)


def format_tsv(top, names, spans, proteins=None, positions=False, annotations=False, cap=None, align=False, seq_type=abi.PROTEIN):
    """kaamer_format_tsv_arrays on a TopResult (or any object with its arrays: n_reported, meta, top_off, top_pid, top_kmatch
    and, with positions, pos_bits_len / pos_off / pos_bits): the TSV rows of the reported hits, formatted on the host
    (search.go:505-554) -> (bytes, line_off u64[entries + 1]).  names: the bytes the records' names lie in (the text of a
    text call); spans: SPAN_DTYPE, one per input record (TopResult.text_spans).  cap: format into a buffer of that many
    bytes instead of one of the needed size -> (bytes written without the NUL, the needed length).
    align: the -aln rows (search.go:556-604), kaamer_format_tsv_aln_arrays -- top.alignments: one per entry, as ALN_DTYPE
    records or dicts with its fields (TopResult.alignments; None: KaamerError E_ARG); seq_type: the request's, whose base
    decides QStart / QEnd."""
    names = names.encode("latin-1") if isinstance(names, str) else bytes(names)
    spans = np.ascontiguousarray(spans, SPAN_DTYPE)
    r = int(top.n_reported)
    meta = np.ascontiguousarray(top.meta, META_DTYPE)
    off = np.ascontiguousarray(top.top_off, np.uint64)
    pid = np.ascontiguousarray(top.top_pid, np.uint32)
    km = np.ascontiguousarray(top.top_kmatch, np.uint32)
    bt = abi.BatchTop()
    bt.n_queries, bt.n_reported, bt.max_results = int(getattr(top, "n_queries", r)), r, int(getattr(top, "max_results", 0))
    bt.q = C.cast(meta.ctypes.data, C.POINTER(abi.QueryMeta))
    bt.top_off = C.cast(off.ctypes.data, C.POINTER(C.c_uint64))
    bt.top_pid = C.cast(pid.ctypes.data, C.POINTER(C.c_uint32))
    bt.top_kmatch = C.cast(km.ctypes.data, C.POINTER(C.c_uint32))
    pl = po = pb = None
    if positions and getattr(top, "pos_bits", None) is not None:
        pl = np.ascontiguousarray(top.pos_bits_len, np.int32)
        po = np.ascontiguousarray(top.pos_off, np.uint64)
        pb = np.ascontiguousarray(top.pos_bits, np.uint64) if len(top.pos_bits) else np.zeros(1, np.uint64)
    ne = int(off[r]) if r else 0
    line_off = np.zeros(ne + 1, np.uint64)
    ph = proteins._h if proteins is not None else None
    alns = None
    if align and getattr(top, "alignments", None) is not None:
        alns = aln_records(top.alignments, ne)
    bitmaps = (pl.ctypes.data if pl is not None else None, po.ctypes.data if po is not None else None, pb.ctypes.data if pb is not None else None)
    name_args = (names, len(names), spans.ctypes.data if len(spans) else None, len(spans), ph)

    def call(buf, n):
        if align:
            rc = int(abi.lib().kaamer_format_tsv_aln_arrays(C.byref(bt), alns.ctypes.data if alns is not None else None, *bitmaps, *name_args, int(seq_type),
                                                            int(bool(positions)), int(bool(annotations)), buf, n, line_off.ctypes.data))
        else:
            rc = int(abi.lib().kaamer_format_tsv_arrays(C.byref(bt), *bitmaps, *name_args, int(bool(positions)), int(bool(annotations)), buf, n,
                                                        line_off.ctypes.data))
        if rc < 0:
            abi.check(rc)
        return rc
    need = call(None, 0)
    if cap is not None:
        buf = C.create_string_buffer(max(int(cap), 1))
        call(buf if cap else None, int(cap))
        return (buf.raw[:min(need, int(cap) - 1)] if cap else b""), need
    buf = C.create_string_buffer(need + 1)
    call(buf, need + 1)
    return buf.raw[:need], line_off


def _sized(fn, *args):
    """need = f(NULL, 0), then the bytes: the convention of the host formatters that cannot fail"""
    need = int(fn(*args, None, 0))
    buf = C.create_string_buffer(need + 1)
    fn(*args, buf, need + 1)
    return buf.raw[:need]


def format_json_header(annotations=False, proteins=None):
    """kaamer_format_json_header: the opening bytes of the JSON response (search.go:672-688) -> bytes"""
    return _sized(abi.lib().kaamer_format_json_header, int(bool(annotations)), proteins._h if proteins is not None else None)


def format_json_trailer():
    """kaamer_format_json_trailer: the closing bytes of the JSON response (search.go:629-632) -> bytes"""
    return _sized(abi.lib().kaamer_format_json_trailer)


def json_escape(data):
    """kaamer_json_escape: the bytes of a string between its quotes, as encoding/json writes them -> bytes"""
    data = bytes(data)
    return _sized(abi.lib().kaamer_json_escape, data, len(data))


def json_protein_value(entry_id=b"", sequence=b"", length=0, features=()):
    """kaamer_json_protein_value: json.Marshal(Protein) of a hand-built entry; features: [(name, value)] -> bytes"""
    names = [bytes(k) for k, _ in features]
    values = b"".join(bytes(v) for _, v in features)
    off = np.zeros(len(names) + 1, np.uint64)
    off[1:] = np.cumsum([len(v) for _, v in features]) if names else 0
    eid, seq = C.create_string_buffer(bytes(entry_id), len(entry_id) + 1), C.create_string_buffer(bytes(sequence), len(sequence) + 1)
    vals = C.create_string_buffer(values, len(values) + 1)
    e = abi.ProteinEntry()
    e.found, e.length = 1, int(length)
    e.entry_id, e.entry_id_len = C.addressof(eid), len(entry_id)
    e.sequence, e.sequence_len = C.addressof(seq), len(sequence)
    e.n_features, e.features = len(names), C.addressof(vals)
    e.feature_off = C.cast(off.ctypes.data, C.POINTER(C.c_uint64))
    arr = (C.c_char_p * max(len(names), 1))(*names)
    return _sized(abi.lib().kaamer_json_protein_value, C.byref(e), arr if names else None)


def format_json(top, names, spans, proteins=None, seqs=None, offsets=None, seq_type=abi.PROTEIN, text_format=0, positions=False, cap=None):
    """kaamer_format_json_arrays on a TopResult (or any object with its arrays: n_reported, meta, trim, top_off, top_pid,
    top_kmatch, orf_aa and, where bitmaps are required, pos_bits_len / pos_off / pos_bits): the JSON objects of the reported
    queries, formatted on the host (search.go:497-503) -> (bytes, obj_off u64[n_reported + 1]).  names / spans: as
    format_tsv takes them.  seqs / offsets: the packed records of a protein request (bytes / u8 array and u64[n + 1]).
    seq_type: the request's; text_format: 0 FASTA records, 1 FASTQ records (Contig); positions: ExtractPositions (protein
    requests only: nucleotide / reads always print them).  top.alignments not None: KaamerError E_ARG.  cap: format into a
    buffer of that many bytes -> (bytes written without the NUL, the needed length)."""
    names = names.encode("latin-1") if isinstance(names, str) else bytes(names)
    spans = np.ascontiguousarray(spans, SPAN_DTYPE)
    r = int(top.n_reported)
    meta = np.ascontiguousarray(top.meta, META_DTYPE)
    off = np.ascontiguousarray(top.top_off, np.uint64)
    pid = np.ascontiguousarray(top.top_pid, np.uint32)
    km = np.ascontiguousarray(top.top_kmatch, np.uint32)
    trim = np.ascontiguousarray(top.trim, np.int32) if getattr(top, "trim", None) is not None and len(top.trim) else None
    orf = np.ascontiguousarray(top.orf_aa, np.uint8) if getattr(top, "orf_aa", None) is not None else np.zeros(0, np.uint8)
    orf = orf if len(orf) else np.zeros(1, np.uint8)
    bt = abi.BatchTop()
    bt.n_queries, bt.n_reported, bt.max_results = int(getattr(top, "n_queries", r)), r, int(getattr(top, "max_results", 0))
    bt.q = C.cast(meta.ctypes.data, C.POINTER(abi.QueryMeta))
    bt.top_off = C.cast(off.ctypes.data, C.POINTER(C.c_uint64))
    bt.top_pid = C.cast(pid.ctypes.data, C.POINTER(C.c_uint32))
    bt.top_kmatch = C.cast(km.ctypes.data, C.POINTER(C.c_uint32))
    bt.orf_aa = C.cast(orf.ctypes.data, C.POINTER(C.c_uint8))
    if trim is not None:
        bt.trim = C.cast(trim.ctypes.data, C.POINTER(C.c_int32))
    pl = po = pb = None
    if getattr(top, "pos_bits", None) is not None:
        pl = np.ascontiguousarray(top.pos_bits_len, np.int32)
        po = np.ascontiguousarray(top.pos_off, np.uint64)
        pb = np.ascontiguousarray(top.pos_bits, np.uint64) if len(top.pos_bits) else np.zeros(1, np.uint64)
    ne = int(off[r]) if r else 0
    alns = aln_records(top.alignments, ne) if getattr(top, "alignments", None) is not None else None
    n_seqs = 0
    if seqs is not None:
        seqs = np.frombuffer(bytes(seqs), np.uint8) if isinstance(seqs, (bytes, bytearray)) else np.ascontiguousarray(seqs, np.uint8)
        seqs = seqs if len(seqs) else np.zeros(1, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        n_seqs = len(offsets) - 1
    obj_off = np.zeros(r + 1, np.uint64)
    args = (C.byref(bt), alns.ctypes.data if alns is not None else None, pl.ctypes.data if pl is not None else None,
            po.ctypes.data if po is not None else None, pb.ctypes.data if pb is not None else None,
            seqs.ctypes.data if n_seqs else None, offsets.ctypes.data if n_seqs else None, n_seqs, names, len(names),
            spans.ctypes.data if len(spans) else None, len(spans), proteins._h if proteins is not None else None, int(seq_type),
            int(text_format), int(bool(positions)))

    def call(buf, n):
        rc = int(abi.lib().kaamer_format_json_arrays(*args, buf, n, obj_off.ctypes.data))
        if rc < 0:
            abi.check(rc)
        return rc
    need = call(None, 0)
    if cap is not None:
        buf = C.create_string_buffer(max(int(cap), 1))
        call(buf if cap else None, int(cap))
        return (buf.raw[:min(need, int(cap) - 1)] if cap else b""), need
    buf = C.create_string_buffer(need + 1)
    call(buf, need + 1)
    return buf.raw[:need], obj_off


# kaamer_alignment as a numpy record
ALN_DTYPE =np.dtype([("identity", np.float32), ("similarity", np.float32), ("length", np.int32), ("mismatches", np.int32),
                      ("gap_openings", np.int32), ("raw", np.int32), ("bitscore", np.float64), ("evalue", np.float64),
                      ("query_start", np.int32), ("query_end", np.int32), ("subject_start", np.int32), ("subject_end", np.int32),
                      ("aln_off", np.uint64), ("status", np.int32), ("reserved", np.int32)])
assert ALN_DTYPE.itemsize == C.sizeof(abi.Alignment)


def aln_records(alignments, n):
    """n kaamer_alignment records from ALN_DTYPE records, or from dicts with (some of) its fields"""
    if isinstance(alignments, np.ndarray) and alignments.dtype == ALN_DTYPE:
        out = np.ascontiguousarray(alignments)
    else:
        out = np.zeros(max(len(alignments), 1), ALN_DTYPE)
        for i, a in enumerate(alignments):
            for k in ALN_DTYPE.names:
                if k in a:
                    out[i][k] = a[k]
    assert len(out) >= n, "%d alignments for %d entries" % (len(out), n)
    return out


PAIR_DTYPE = np.dtype([(k, np.int32) for k in ("status", "n_ops", "start_i", "start_j", "end_i", "end_j", "identical", "similar", "mismatches",
                                                "gap_openings", "raw")] + [("query_len", np.uint32), ("off", np.uint64), ("entry", np.uint32),
                                                                           ("subject_len", np.uint32)])
assert PAIR_DTYPE.itemsize == C.sizeof(abi.AlignPair)


def align_finish_pairs(pairs, number_of_aa, sub_matrix="blosum62", gap_open=11, gap_extend=1):
    """kaamer_align_finish_pairs: PAIR_DTYPE records (kaamer_align_pair) -> ALN_DTYPE records, the floats and coordinates a
    result of the aligning calls carries for them"""
    pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
    out = np.zeros(max(len(pairs), 1), ALN_DTYPE)
    abi.check(abi.lib().kaamer_align_finish_pairs(pairs.ctypes.data if len(pairs) else None, len(pairs), int(number_of_aa), sub_matrix.encode(),
                                                  int(gap_open), int(gap_extend), out.ctypes.data))
    return out[:len(pairs)]


def format_double(value, mode):
    """kaamer_format_double: a float64 as the -aln rows print EValue (mode 0: "%e") or BitScore (mode 1: "%.2f") -> bytes"""
    return _sized(abi.lib().kaamer_format_double, float(value), int(mode))


def format_doubles_device(d_values_ptr, n, mode, d_out_ptr):
    """kaamer_tsv_format_doubles_device: n float64 at a device address, printed by the device functions of the -aln stage
    into 32-byte slots at d_out_ptr"""
    abi.check(abi.lib().kaamer_tsv_format_doubles_device(C.c_void_p(d_values_ptr), int(n), int(mode), C.c_void_p(d_out_ptr)))


def _geometry(fn, names=("tile", "window", "store", "threads")):
    """a geometry getter of the library, which fills len(names) u32 -> dict"""
    g = (C.c_uint32 * len(names))()
    fn(g)
    return dict(zip(names, (int(v) for v in g)))


def scan_geometry():
    """kaamer_scan_geometry -> dict(block, items, tile, single_max): threads per workgroup of the workspace's prefix scan,
    counts per thread, counts per tile, and the greatest bound the one-workgroup form takes (above it: the tiled launches)"""
    return _geometry(abi.lib().kaamer_scan_geometry, ("block", "items", "tile", "single_max"))


def tsv_geometry():
    """kaamer_tsv_geometry -> dict(tile, window, store, threads): queries per tile of the write pass, bytes per LDS window
    (windows lie on multiples of it in the output), bytes a lane stores at once, threads per workgroup"""
    return _geometry(abi.lib().kaamer_tsv_geometry)


class _RowsStage(_Handle):
    """what TsvStage and JsonStage share: kaamer_{_KIND}_stage_create / _free and kaamer_{_KIND}_rows_finish"""
    _KIND = None

    def __init__(self, index, max_queries, max_units):
        self.index = index
        self._FREE = "kaamer_%s_stage_free" % self._KIND
        super().__init__(_new(getattr(abi.lib(), "kaamer_%s_stage_create" % self._KIND), index._h, int(max_queries), int(max_units)))

    def finish(self, stream=0):
        c = (C.c_uint64 * 2)()
        rc = getattr(abi.lib(), "kaamer_%s_rows_finish" % self._KIND)(self._h, C.c_void_p(stream), c)
        if rc:
            e = abi.error(rc)
            e.counts = (int(c[0]), int(c[1]))
            raise e
        return int(c[0]), int(c[1])


class TsvStage(_RowsStage):
    """kaamer_tsv_stage_*: the buffers of the device stage that writes the TSV rows, for up to max_queries queries and
    max_lines rows (needs Index.attach_subject_text)"""
    _KIND = "tsv"

    def __init__(self, index, max_queries, max_lines):
        super().__init__(index, max_queries, max_lines)

    def rows_device(self, rows_in, d_out_ptr, out_cap, stream=0):
        """kaamer_tsv_rows_device (rows_in: abi.TsvRowsIn of raw device addresses) -> abi.TsvRowsResult"""
        r = abi.TsvRowsResult()
        abi.check(abi.lib().kaamer_tsv_rows_device(self._h, C.byref(rows_in), C.c_void_p(d_out_ptr), int(out_cap), C.c_void_p(stream), C.byref(r)))
        return r

    def aln_rows_device(self, rows_in, alns, d_out_ptr, out_cap, sub_matrix="blosum62", gap_open=11, gap_extend=1, seq_type=abi.PROTEIN,
                        stream=0):
        """kaamer_tsv_aln_rows_device (rows_in: abi.TsvRowsIn, alns: abi.TopnAlignments, both of raw device addresses)
        -> abi.TsvRowsResult"""
        o = abi.TsvAlnOpts()
        o.sub_matrix = sub_matrix.encode() if isinstance(sub_matrix, str) else sub_matrix
        o.gap_open, o.gap_extend, o.seq_type = int(gap_open), int(gap_extend), int(seq_type)
        r = abi.TsvRowsResult()
        abi.check(abi.lib().kaamer_tsv_aln_rows_device(self._h, C.byref(rows_in), C.byref(alns), C.byref(o), C.c_void_p(d_out_ptr), int(out_cap),
                                                       C.c_void_p(stream), C.byref(r)))
        return r

    def aln_info(self):
        """kaamer_tsv_aln_info -> dict(outside: pairs of the last -aln call with a raw score outside the table, table: raw
        scores it holds, tables: tables filled so far)"""
        return _info(abi.lib().kaamer_tsv_aln_info, self._h, 4, ("outside", "table", "tables"))

    def finish(self, stream=0):
        """kaamer_tsv_rows_finish -> (rows, bytes); KaamerError E_CAPACITY (with .counts = what was needed) when they did not
        fit, E_RANGE after aln_rows_device when a raw score lies outside the table (the batch is the host formatter's)"""
        return super().finish(stream)


def json_geometry():
    """kaamer_json_geometry -> dict(tile, window, store, threads): queries per tile, bytes of a wave's LDS buffer, bytes a lane
    stores at once, threads per workgroup"""
    return _geometry(abi.lib().kaamer_json_geometry)


class JsonStage(_RowsStage):
    """kaamer_json_stage_*: the buffers of the device stage that writes the JSON objects, for up to max_queries queries and
    max_objects objects (needs Index.attach_subject_json)"""
    _KIND = "json"

    def __init__(self, index, max_queries, max_objects):
        super().__init__(index, max_queries, max_objects)

    def rows_device(self, rows_in, d_out_ptr, out_cap, stream=0):
        """kaamer_json_rows_device (rows_in: abi.JsonRowsIn of raw device addresses) -> abi.JsonRowsResult"""
        r = abi.JsonRowsResult()
        abi.check(abi.lib().kaamer_json_rows_device(self._h, C.byref(rows_in), C.c_void_p(d_out_ptr), int(out_cap), C.c_void_p(stream), C.byref(r)))
        return r

    def finish(self, stream=0):
        """kaamer_json_rows_finish -> (objects, bytes); KaamerError E_CAPACITY (with .counts = what was needed) when they did
        not fit"""
        return super().finish(stream)


def _align_args(align):
    """(sub_matrix, gap_open, gap_extend, want_text) of an `align` dict (Index.search_top)"""
    return (str(align.get("sub_matrix", "blosum62")).encode(), int(align.get("gap_open", 11)), int(align.get("gap_extend", 1)),
            int(bool(align.get("text", True))))


def _drive_file(fn, args, cb_type, chunk_args, on_chunk):
    """one whole-file driver: fn(*args, cb, user, total), its callback (a cb_type) wrapped around on_chunk -> summed counters.
    chunk_args: what the callback receives behind `user` -> on_chunk's arguments.  An exception of on_chunk stops the run and
    is raised here"""
    err = []

    def cb(user, *chunk):
        try:
            if on_chunk is not None:
                on_chunk(*chunk_args(*chunk))
            return 0
        except BaseException as e:  # noqa: BLE001  (must not propagate through the C frames)
            err.append(e)
            return 1
    c = abi.Counters()
    cfn = cb_type(cb)
    rc = fn(*args, C.cast(cfn, C.c_void_p), None, C.byref(c))
    if err:
        raise err[0]
    abi.check(rc)
    return c.as_dict()


def _search_file(ix, path, fmt, seq_type, top, chunk_seqs, chunk_bytes, in_flight, strict, on_chunk, want_positions, align):
    """the three whole-file calls of the host reader: kaamer_sharded_search_file on a ShardedIndex; on a Replicas set
    kaamer_search_file_opts, or kaamer_search_file, which has no such arguments, when neither bitmaps nor alignments are asked
    for.  on_chunk(first_seq, reads_handle, TopResult)"""
    opts = (int(bool(want_positions)), int(align is not None)) + (_align_args(align) if align is not None else (None, 0, 0, 0))
    if isinstance(ix, ShardedIndex):
        fn = abi.lib().kaamer_sharded_search_file
    elif want_positions or align is not None:
        fn = abi.lib().kaamer_search_file_opts
    else:
        fn, opts = abi.lib().kaamer_search_file, ()
    args = (ix._h, str(path).encode(), 1 if fmt == "fastq" else 0, int(strict), seq_type, *top, *opts, chunk_seqs, chunk_bytes, in_flight)
    return _drive_file(fn, args, Replicas.CHUNK_CB, lambda first, reads, top_: (int(first), C.c_void_p(reads), TopResult(top_)), on_chunk)


class _Ticket(_Handle):
    """One batch in flight on an Index or (sharded=True) a ShardedIndex: wait() exactly once -- the ticket is empty after it,
    even if it raises -- and a ticket dropped unwaited is discarded: its slot goes back to the pool instead of staying busy
    for good.  A subclass names its wait and discard symbols, the result's C type and what takes it."""
    _WAIT = _DISCARD = _OUT = _take = None

    def __init__(self, handle, sharded=False):
        super().__init__(handle)
        self._sharded = sharded

    def _symbol(self, name):
        return getattr(abi.lib(), "kaamer_%s%s" % ("sharded_" if self._sharded else "", name))

    def wait(self):
        out = C.POINTER(self._OUT)()
        h, self._h = self._h, None
        abi.check(self._symbol(self._WAIT)(h, C.byref(out)))
        return self._take(out)

    def _free(self, h):
        self._symbol(self._DISCARD)(h)

    discard = _Handle.close


class FullTicket(_Ticket):
    """one full-hit-list batch in flight (kaamer_full_ticket / kaamer_sharded_full_ticket); wait() exactly once,
    discarded when dropped"""
    _WAIT, _DISCARD, _OUT, _take = "wait_batch", "full_ticket_discard", abi.BatchOut, staticmethod(BatchResult)


class TopTicket(_Ticket):
    """one batch in flight (kaamer_ticket / kaamer_sharded_ticket); wait() exactly once.  A ticket dropped unwaited is
    discarded (kaamer_ticket_discard): its slot goes back to the pool instead of staying busy for good."""
    _WAIT, _DISCARD, _OUT, _take = "wait_batch_top", "ticket_discard", abi.BatchTop, staticmethod(_take_top)


class TopStream(_Handle):
    """kaamer_stream_* / kaamer_replica_stream_* / kaamer_sharded_stream_*: a FIFO of batches with fixed options (push
    chunk i + 1 while chunk i is searched) on an Index, a Replicas set or a ShardedIndex"""

    def __init__(self, index, seq_type, min_k_ratio, min_k_match, max_results, want_positions=False, align=None):
        L, kind, top = abi.lib(), index._STREAM, (min_k_ratio, min_k_match, max_results)
        self._fn = {k: getattr(L, "kaamer_%s_%s" % (kind, k)) for k in ("push", "pop", "pending", "close")}
        self.index = index
        if align is not None:
            h = _new(getattr(L, "kaamer_%s_open_aln_flat" % kind), index._h, seq_type, *top, int(bool(want_positions)), *_align_args(align))
        elif want_positions:
            h = _new(getattr(L, "kaamer_%s_open_pos_flat" % kind), index._h, seq_type, *top)
        elif kind == "stream":   # the struct form
            to = abi.TopnOpts(*top, 0, None, None, 0, 0)
            h = _new(L.kaamer_stream_open, index._h, seq_type, C.byref(to))
        else:
            h = _new(getattr(L, "kaamer_%s_open_flat" % kind), index._h, seq_type, *top)
        super().__init__(h)

    def push(self, buf, offs):
        """-> False when every slot (set) is busy with this stream's own chunks (pop first), True when the chunk was taken"""
        buf, offs, batch = packed_batch(packed=(buf, offs))
        rc = self._fn["push"](self._h, *batch)
        if rc == abi.E_BUSY:
            return False
        abi.check(rc)
        return True

    def pop(self):
        out = C.POINTER(abi.BatchTop)()
        abi.check(self._fn["pop"](self._h, C.byref(out)))
        return _take_top(out)

    @property
    def pending(self):
        return int(self._fn["pending"](self._h))

    def _free(self, h):
        self._fn["close"](h)


class Workspace(_Handle):
    """Reusable device buffers for the device-resident call."""
    _FREE = "kaamer_workspace_free"

    def __init__(self, index, max_seq_bytes, max_seqs, max_queries=0, max_hits=0, g_tier_slots=0, seq_type=abi.PROTEIN,
                 first_pos=0, want_positions=False, max_pos_words=0, compact=False, concurrent_batches=0):
        self.index = index
        self.seq_type = seq_type
        o = abi.WorkspaceOpts(max_seq_bytes, max_seqs, max_queries, max_hits,
                              g_tier_slots, seq_type, first_pos, int(want_positions), int(compact), max_pos_words,
                              int(concurrent_batches), 0)
        super().__init__(_new(abi.lib().kaamer_workspace_create, index._h, C.byref(o)))

    def search_device(self, d_seqs_ptr, d_offsets_ptr, n_seqs, seq_bytes, seq_type=None, stream=0):
        """Enqueue one batch; pointers are raw device addresses (e.g. tensor.data_ptr()),
        `stream` a raw hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)."""
        if seq_type is None:
            seq_type = self.seq_type
        r = abi.DeviceResult()
        abi.check(abi.lib().kaamer_search_device(self.index._h, self._h, d_seqs_ptr, d_offsets_ptr, n_seqs,
                                                 seq_bytes, seq_type, C.c_void_p(stream), C.byref(r)))
        return r

    def merge_device(self, d_ent_off_ptr, d_pid_ptr, d_km_ptr, d_fp_ptr, n_queries, n_entries, stream=0):
        """Merge partial hit lists (sharded index); same result object as search_device."""
        r = abi.DeviceResult()
        abi.check(abi.lib().kaamer_merge_device(self._h, d_ent_off_ptr, d_pid_ptr, d_km_ptr, d_fp_ptr, n_queries,
                                                n_entries, C.c_void_p(stream), C.byref(r)))
        return r

    def topn_device(self, min_k_ratio=0.05, min_k_match=10, max_results=10, best_start_codon=False,
                    d_size_in_kmer_ptr=None, stream=0, orf_source=None, q_first=0, q_stride=1):
        """sortMapByValue + (SetBestStartCodon) + FilterResults of the last search/merge, on the device;
        orf_source: the workspace whose queries the (merged) results belong to (result i = its query q_first + i q_stride)"""
        o = abi.TopnOpts(min_k_ratio, min_k_match, max_results, int(best_start_codon), d_size_in_kmer_ptr,
                         orf_source._h if orf_source is not None else None, q_first, q_stride)
        r = abi.TopnResult()
        abi.check(abi.lib().kaamer_topn_device(self._h, C.byref(o), C.c_void_p(stream), C.byref(r)))
        return r

    def topn_positions_device(self, top, max_pos_words=0, stream=0):
        """kaamer_topn_positions_device: the PositionHits bitmaps of the hits the last topn_device call (`top`, its
        result) kept, left on the device -> abi.TopnPositions (d_pos_base[n + 1], d_pos_bits_len[n], d_pos_bits)"""
        r = abi.TopnPositions()
        abi.check(abi.lib().kaamer_topn_positions_device(self.index._h, self._h, C.byref(top), int(max_pos_words),
                                                         C.c_void_p(stream), C.byref(r)))
        return r

    def topn_align_device(self, top, sub_matrix="blosum62", gap_open=11, gap_extend=1, max_query_len=0, max_pairs=0, stream=0):
        """kaamer_topn_align_device: every hit the last topn_device call (`top`, its result) kept, aligned with its query
        against the index's attached protein table, left on the device -> abi.TopnAlignments (d_pair_off[n + 1],
        d_pairs: abi.AlignPair records)"""
        o = abi.TopnAlignOpts(sub_matrix.encode(), gap_open, gap_extend, int(max_query_len), 0, int(max_pairs))
        r = abi.TopnAlignments()
        abi.check(abi.lib().kaamer_topn_align_device(self.index._h, self._h, C.byref(top), C.byref(o), C.c_void_p(stream), C.byref(r)))
        return r

    def set_count_stream(self, stream):
        """kaamer_workspace_set_count_stream: the counting stage of this workspace's batches runs on `stream` (raw hipStream_t; 0 / None: off)"""
        abi.check(abi.lib().kaamer_workspace_set_count_stream(self._h, C.c_void_p(stream or 0)))

    @property
    def query_capacity(self):
        return int(abi.lib().kaamer_workspace_query_capacity(self._h))

    def exchange_pack(self, layout, d_send_ptr, stream=0):
        abi.check(abi.lib().kaamer_exchange_pack(self._h, C.byref(layout), d_send_ptr, C.c_void_p(stream)))

    def exchange_stats_positions(self, back=0):
        """-> (bitmap words the largest block between any pair of ranks needed, a bitmap section overflowed) of the merge
        `back` calls ago on this workspace (kaamer_exchange_stats_positions)"""
        return tuple(_u64s(abi.lib().kaamer_exchange_stats_positions, 2, self._h, back))

    def exchange_stats(self, back=0):
        """-> (merge sequence number, queries of the batch, entries the largest block any pair of ranks needed, overflow)
        of the merge `back` calls ago on this workspace; the same figures on every rank"""
        return tuple(_u64s(abi.lib().kaamer_exchange_stats, 4, self._h, back))

    def exchange_merge(self, layout, d_recv_ptr, stream=0):
        r = abi.DeviceResult()
        abi.check(abi.lib().kaamer_exchange_merge(self._h, C.byref(layout), d_recv_ptr, C.c_void_p(stream), C.byref(r)))
        return r

    def finish(self, stream=0):
        c = abi.Counters()
        abi.check(abi.lib().kaamer_workspace_finish(self._h, C.c_void_p(stream), C.byref(c)))
        return c.as_dict()

    def kernel_ms_sum(self):
        """dict(probe_ms, count_ms, total_ms, calls) summed since reset_timers()."""
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
        abi.check(abi.lib().kaamer_workspace_kernel_ms_sum(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return dict(probe_ms=float(a.value), count_ms=float(b.value), total_ms=float(c.value), calls=int(n.value))

    def reset_timers(self):
        abi.lib().kaamer_workspace_reset_timers(self._h)

    def set_timing(self, every):
        """0: no kernel timers (default); k: HIP events around the kernels of every k-th call"""
        abi.lib().kaamer_workspace_set_timing(self._h, int(every))


def _reads_to_arrays(h):
    """a kaamer_reads handle -> (seqs u8, offsets u64, size_in_kmer, names bytes, name offsets, plus_strand), copied"""
    L = abi.lib()
    n = L.kaamer_reads_count(h)
    offs = np.ctypeslib.as_array(L.kaamer_reads_offsets(h), shape=(n + 1,)).copy()
    noff = np.ctypeslib.as_array(L.kaamer_reads_name_offsets(h), shape=(n + 1,)).copy()
    seqs = np.ctypeslib.as_array(L.kaamer_reads_seqs(h), shape=(int(offs[n]),)).copy() if offs[n] else np.zeros(0, np.uint8)
    names = bytes(np.ctypeslib.as_array(C.cast(L.kaamer_reads_names(h), C.POINTER(C.c_uint8)), shape=(int(noff[n]),))) if noff[n] else b""
    size = np.ctypeslib.as_array(L.kaamer_reads_size_in_kmer(h), shape=(n,)).copy() if n else np.zeros(0, np.int32)
    plus = np.ctypeslib.as_array(L.kaamer_reads_plus_strand(h), shape=(n,)).copy() if n else np.zeros(0, np.int32)
    return seqs, offs, size, names, noff, plus


class Reader(_Handle):
    """kaamer_reader_*: GetQueriesFasta / GetQueriesFastq over a file in chunks (gzip inflated incrementally)"""
    _FREE = "kaamer_reader_close"

    def __init__(self, path=None, fmt="fastq", strict=False, fd=None):
        f = 1 if fmt == "fastq" else 0
        if fd is not None:
            super().__init__(_new(abi.lib().kaamer_reader_open_fd, fd, f, int(strict)))
        else:
            super().__init__(_new(abi.lib().kaamer_reader_open, str(path).encode(), f, int(strict)))

    def next_handle(self, max_seqs, max_bytes):
        """-> a raw kaamer_reads handle (free with kaamer_reads_free), or None at the end"""
        r = _new(abi.lib().kaamer_reader_next, self._h, max_seqs, max_bytes)
        if abi.lib().kaamer_reads_count(r) == 0 and self.done:
            abi.lib().kaamer_reads_free(r)
            return None
        return r

    def next(self, max_seqs=1 << 20, max_bytes=1 << 28):
        """-> (seqs, offsets, size_in_kmer, names, name_offsets, plus_strand) of the next chunk, or None at the end"""
        r = self.next_handle(max_seqs, max_bytes)
        if r is None:
            return None
        try:
            return _reads_to_arrays(r)
        finally:
            abi.lib().kaamer_reads_free(r)

    @property
    def done(self):
        return bool(abi.lib().kaamer_reader_done(self._h))

    @property
    def records(self):
        return int(abi.lib().kaamer_reader_records(self._h))

    def records_list(self, max_seqs=1 << 20, max_bytes=1 << 28):
        """every record of the file as parse_reads returns them (tests)"""
        out = []
        while True:
            c = self.next(max_seqs, max_bytes)
            if c is None:
                return out
            out += _read_records(c)


def _read_records(arrays):
    """what _reads_to_arrays returns -> list of dict(seq, name, size, plus)"""
    seqs, offs, size, names, noff, plus = arrays
    sb = bytes(seqs)
    return [dict(seq=sb[int(offs[i]):int(offs[i + 1])].decode("latin-1"), name=names[int(noff[i]):int(noff[i + 1])].decode("latin-1"),
                 size=int(size[i]), plus=bool(plus[i])) for i in range(len(size))]


def parse_reads(text, fmt="fasta"):
    """GetQueriesFasta / GetQueriesFastq on a text buffer -> list of dict(seq, name, size, plus)"""
    data = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    h = _new(abi.lib().kaamer_parse_fasta if fmt == "fasta" else abi.lib().kaamer_parse_fastq, data, len(data))
    try:
        return _read_records(_reads_to_arrays(h))
    finally:
        abi.lib().kaamer_reads_free(h)


def text_parser_geometry():
    """kaamer_text_parser_geometry -> dict(piece, wave_step, tile, lines): the tiling of the device parser's kernels"""
    return _geometry(abi.lib().kaamer_text_parser_geometry, ("piece", "wave_step", "tile", "lines"))


def text_cut_fastq(text):
    """kaamer_text_cut_fastq: the greatest p in [1, len) with text[p-1] == '\\n' and text[p] == '@'; 0: none"""
    data = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    return int(abi.lib().kaamer_text_cut_fastq(data, len(data)))


def text_cut_fasta(text):
    """kaamer_text_cut_fasta: the greatest p in [1, len) with text[p-1] == '\\n', text[p] == '>' and a sequence line (complete
    or not) in text[p:]; 0: none"""
    data = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    return int(abi.lib().kaamer_text_cut_fasta(data, len(data)))


def text_cut_embl(text):
    """kaamer_text_cut_embl: the greatest p <= len such that text[:p] ends with the line end of a line that is exactly "//"
    after the '\\r' drop (a final "//" without '\\n' counts as the text's last line: p = len); 0: none"""
    data = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    return int(abi.lib().kaamer_text_cut_embl(data, len(data)))


def text_cut_gbk(text):
    """where a GBK text may be cut (Proteins.from_gbk on a device): its entries end as EMBL's do, so this is text_cut_embl"""
    return text_cut_embl(text)


def _hip_runtime():
    """the HIP runtime torch loaded (device copies of the tools below)"""
    import torch
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


class TextParser(_Handle):
    """kaamer_text_parser_*: GetQueriesFastq / GetQueriesFasta on the device, for texts of up to max_text_bytes with up to
    max_records records (None: as many as such a text can hold) and max_lines lines (None: the FASTQ rule,
    max_text_bytes / 16 + 4 max_records + 1024; kaamer_text_parser_create_lines otherwise)"""
    _FREE = "kaamer_text_parser_free"

    def __init__(self, max_text_bytes, max_records=None, device=0, max_lines=None):
        self.device = device
        self.max_text_bytes = int(max_text_bytes)
        if max_records is None:
            max_records = self.max_text_bytes // 2 + 1
        if max_lines is None:
            super().__init__(_new(abi.lib().kaamer_text_parser_create, device, self.max_text_bytes, int(max_records)))
        else:
            super().__init__(_new(abi.lib().kaamer_text_parser_create_lines, device, self.max_text_bytes, int(max_records), int(max_lines)))

    def parse_device(self, d_text_ptr, n_bytes, stream=0, fmt="fastq", upper_last=False):
        """kaamer_parse_fastq_device (fmt "fasta": kaamer_parse_fasta_device) + kaamer_text_parser_finish on a device
        buffer -> abi.TextParseResult"""
        if fmt == "fasta":
            abi.check(abi.lib().kaamer_parse_fasta_device(self._h, d_text_ptr, n_bytes, int(bool(upper_last)), stream))
        elif fmt == "fastq":
            abi.check(abi.lib().kaamer_parse_fastq_device(self._h, d_text_ptr, n_bytes, stream))
        else:
            raise ValueError("fmt is 'fastq' or 'fasta'")
        r = abi.TextParseResult()
        abi.check(abi.lib().kaamer_text_parser_finish(self._h, stream, C.byref(r)))
        return r

    def parse(self, text, fmt="fastq", upper_last=False):
        """text (bytes) -> dict(seqs u8, offsets u64, spans (SPAN_DTYPE), n_lines): uploaded, parsed, copied back.
        fmt "fasta": GetQueriesFasta; upper_last: more input follows the text, its last record is upper-cased too"""
        import torch
        data = text.encode("latin-1") if isinstance(text, str) else bytes(text)
        with torch.cuda.device(self.device):
            d = torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            r = self.parse_device(d.data_ptr(), len(data), fmt=fmt, upper_last=upper_last)
            hip = _hip_runtime()
            n = int(r.n_records)
            offs = np.empty(n + 1, np.uint64)
            spans = np.empty(n, SPAN_DTYPE)
            seqs = np.empty(int(r.seq_bytes), np.uint8)
            for arr, ptr in ((offs, r.d_offsets), (spans, r.d_spans), (seqs, r.d_seqs)):
                if arr.nbytes:
                    assert hip.hipMemcpy(arr.ctypes.data, C.c_void_p(ptr), arr.nbytes, 2) == 0
            del d
        return dict(seqs=seqs, offsets=offs, spans=spans, n_lines=int(r.n_lines))


def parse_fastq_device(text, device=0):
    """GetQueriesFastq on the device (tests and tools) -> dict(seqs, offsets, spans, n_lines) as numpy arrays; spans index
    the text (SPAN_DTYPE: name_off, name_len, seq_off, seq_len)"""
    data = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    p = TextParser(len(data), device=device)
    try:
        return p.parse(data)
    finally:
        p.close()


def parse_fasta_device(text, upper_last=False, device=0):
    """GetQueriesFasta on the device (tests and tools) -> dict(seqs, offsets, spans, n_lines) as numpy arrays.  A record's
    span covers text[seq_off : seq_off + seq_len] from its first to its last kept byte, line breaks included"""
    data = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    p = TextParser(len(data), device=device)
    try:
        return p.parse(data, fmt="fasta", upper_last=upper_last)
    finally:
        p.close()


BGZF_BLOCK_DTYPE = np.dtype([("comp_off", "<u8"), ("comp_len", "<u4"), ("isize", "<u4"), ("crc", "<u4"), ("reserved", "<u4")])   # kaamer_bgzf_block


def bgzf_scan(data):
    """kaamer_bgzf_scan (CPU): the BGZF blocks at the start of `data` (bytes), found without inflating ->
    (blocks as a BGZF_BLOCK_DTYPE array, consumed).  consumed == len(data): the bytes are whole BGZF blocks."""
    data = bytes(data)
    n, used = C.c_uint64(), C.c_uint64()
    L = abi.lib()
    abi.check(L.kaamer_bgzf_scan(data, len(data), None, 0, C.byref(n), C.byref(used)))
    blocks = np.zeros(int(n.value), BGZF_BLOCK_DTYPE)
    if len(blocks):
        abi.check(L.kaamer_bgzf_scan(data, len(data), blocks.ctypes.data, len(blocks), C.byref(n), C.byref(used)))
    return blocks, int(used.value)


def inflater_geometry():
    """kaamer_inflater_geometry -> dict(crc_segment, blocks_per_workgroup, cut_tile, scan_threads)"""
    return _geometry(abi.lib().kaamer_inflater_geometry, ("crc_segment", "blocks_per_workgroup", "cut_tile", "scan_threads"))


def text_cut_fastq_device(text, device=0):
    """kaamer_text_cut_fastq_device of `text` (bytes), uploaded for the call (tests)"""
    import torch
    data = bytes(text)
    with torch.cuda.device(device):
        d = torch.frombuffer(bytearray(data) if data else bytearray(1), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        cut = C.c_uint64()
        abi.check(abi.lib().kaamer_text_cut_fastq_device(device, d.data_ptr(), len(data), None, C.byref(cut)))
        del d
    return int(cut.value)


class Inflater(_Handle):
    """kaamer_inflater_*: BGZF blocks inflated on the device, one wave per block, for calls of up to max_blocks blocks
    within max_comp_bytes compressed bytes"""
    _FREE = "kaamer_inflater_free"

    def __init__(self, max_comp_bytes, max_blocks, device=0):
        self.device = device
        self.max_comp_bytes = int(max_comp_bytes)
        self.max_blocks = int(max_blocks)
        super().__init__(_new(abi.lib().kaamer_inflater_create, device, self.max_comp_bytes, self.max_blocks))

    def inflate_device(self, d_comp_ptr, comp_bytes, d_blocks_ptr, n_blocks, d_out_ptr, out_cap, stream=0):
        """kaamer_inflate_bgzf_device + kaamer_inflater_finish on device buffers -> abi.InflateResult"""
        abi.check(abi.lib().kaamer_inflate_bgzf_device(self._h, d_comp_ptr, comp_bytes, d_blocks_ptr, n_blocks, d_out_ptr, out_cap, stream))
        r = abi.InflateResult()
        abi.check(abi.lib().kaamer_inflater_finish(self._h, stream, C.byref(r)))
        return r

    def inflate(self, comp_tensor, blocks, out_offset=0):
        """comp_tensor: the compressed bytes (a uint8 tensor on the device, or bytes: uploaded); blocks: BGZF_BLOCK_DTYPE
        array (bgzf_scan).  The text goes to a fresh device buffer `out_offset` bytes behind its start.
        -> dict(text u8 array, status u32 array, n_bad, first_bad, out_bytes)"""
        import torch
        blocks = np.ascontiguousarray(blocks, dtype=BGZF_BLOCK_DTYPE)
        total = int(blocks["isize"].astype(np.uint64).sum())
        with torch.cuda.device(self.device):
            comp_bytes = int(comp_tensor.numel()) if torch.is_tensor(comp_tensor) else len(bytes(comp_tensor))
            if not torch.is_tensor(comp_tensor):
                comp_tensor = torch.frombuffer(bytearray(bytes(comp_tensor)) or bytearray(1), dtype=torch.uint8).cuda()
            d_blocks = torch.frombuffer(bytearray(blocks.tobytes()) or bytearray(24), dtype=torch.uint8).cuda()
            d_out = torch.full((out_offset + total + 64,), 0xEE, dtype=torch.uint8, device="cuda")   # guard bytes on both sides
            torch.cuda.synchronize()
            r = self.inflate_device(comp_tensor.data_ptr(), comp_bytes, d_blocks.data_ptr(), len(blocks), d_out.data_ptr() + out_offset, total)
            status = np.empty(len(blocks), np.uint32)
            if len(blocks):
                assert _hip_runtime().hipMemcpy(status.ctypes.data, C.c_void_p(r.d_status), status.nbytes, 2) == 0
            whole = d_out.cpu().numpy()
        return dict(text=whole[out_offset:out_offset + total].copy(), guard=(whole[:out_offset].copy(), whole[out_offset + total:].copy()),
                    status=status, n_bad=int(r.n_bad), first_bad=int(r.first_bad), first_bad_status=int(r.first_bad_status), out_bytes=int(r.out_bytes))


def align_pairs(seqs=None, packed=None, pairs=(), number_of_aa=0, sub_matrix="blosum62", gap_open=11, gap_extend=1, device=0):
    """kaamer_align_pairs: align.Align (align.go:46-161) for every (query index, subject index) pair -> list of dicts
    (None where the reference keeps an empty AlignmentResult: "No matrix found"; a ValueError-like status is returned as
    {"status": n})"""
    buf, offs, batch = packed_batch(seqs, packed)
    pq = np.ascontiguousarray([p[0] for p in pairs], dtype=np.uint32)
    ps = np.ascontiguousarray([p[1] for p in pairs], dtype=np.uint32)
    L = abi.lib()
    h = _new(L.kaamer_align_pairs, device, *batch, pq.ctypes.data if len(pq) else None, ps.ctypes.data if len(ps) else None, len(pq),
             int(number_of_aa), sub_matrix.encode(), gap_open, gap_extend)
    try:
        n = L.kaamer_alignments_count(h)
        items = L.kaamer_alignments_items(h)
        text = L.kaamer_alignments_text(h)
        out = []
        for i in range(n):
            a = items[i]
            if a.status == 1:
                out.append(None)
                continue
            d = {k: getattr(a, k) for k, _ in abi.Alignment._fields_ if k not in ("aln_off", "reserved")}
            ln, off = a.length, a.aln_off
            raw = C.string_at(C.addressof(text.contents) + off, 3 * ln) if ln else b""
            d["aln"] = (raw[:ln].decode("latin-1"), raw[ln:2 * ln].decode("latin-1"), raw[2 * ln:].decode("latin-1"))
            out.append(d)
        return out
    finally:
        L.kaamer_alignments_free(h)
