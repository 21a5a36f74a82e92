"""sbam_load_record_tags: selected tags of decoded records as typed device columns, against sbam.sam.find_tags per record
(itself pinned by the reference's 2.sam and 5k.sam and by the core replay, tests/test_record_tags_host.py).

* 2.bam and 5k.bam, the 18-tag query with bytes for every entry, split sizes 100 KiB and one split; `rel` against the
  aux column of load_record_fields;
* hand-built records inserted into 2.bam's stream (handmade_tags): every type and extreme, name and value traps, the
  lane / wave threshold, the wave's NUL search, values larger than any LDS stage, every record alignment;
* batches, repeats, 1- and 32-tag queries, byte-column subsets, coexistence with load_record_fields;
* state, argument and malformed-record errors; `cli tags`; the synthetic file in both read-length modes."""
import ctypes
import os
import struct

import numpy as np
import pytest

from conftest import FIXTURES, fixture_bytes
from test_eager_wave import bgzf
from test_record_fields import _rand_record, record
from test_record_tags_host import (HAND_QUERY, LONG, QUERY18, aux_of, big_lists, golden_table, hand_lists,
                                   malformed_lists)
from test_sam_text import decoded, record_chain, ref_fields, stream_header

gpu = pytest.mark.gpu


def want_columns(auxs, tags, bytes_for):
    """What load_record_tags must return for records with these tag bytes: find_tags per record, as arrays."""
    from sbam import sam
    n, q = len(auxs), len(tags)
    ty, sub = np.zeros((q, n), np.uint8), np.zeros((q, n), np.uint8)
    rel, val = np.full((q, n), -1, np.int32), np.zeros((q, n), np.int64)
    raws = {t: [] for t in bytes_for}
    for k, aux in enumerate(auxs):
        for j, g in enumerate(sam.find_tags(aux, tags)):
            if g is not None:
                ty[j, k], sub[j, k], rel[j, k], val[j, k] = ord(g[0]), ord(g[1]) if g[1] else 0, g[2], g[3]
            if tags[j] in raws:
                raws[tags[j]].append(g[4] if g is not None else b"")
    off = {t: np.concatenate([[0], np.cumsum([len(r) for r in raws[t]], dtype=np.int64)]).astype(np.int64) for t in raws}
    data = {t: np.frombuffer(b"".join(raws[t]), np.uint8) for t in raws}
    return ty, sub, rel, val, off, data


def assert_tags(got, auxs, tags, bytes_for, what=""):
    ty, sub, rel, val, off, data = want_columns(auxs, tags, bytes_for)
    assert got.n == len(auxs) and got.tags == tuple(tags)
    for name, g, w in (("type", got.type, ty), ("sub", got.sub, sub), ("rel", got.rel, rel), ("value", got.value, val)):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{what} {name}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what} {name}: {len(bad)} differ, first (tag, record) {bad[0]}: {g[tuple(bad[0])]} vs {w[tuple(bad[0])]}"
    assert set(got.bytes_off) == set(got.bytes) == set(bytes_for), what
    for t in bytes_for:
        assert np.array_equal(got.bytes_off[t], off[t]), f"{what} bytes_off[{t}]"
        assert np.array_equal(got.bytes[t], data[t]), f"{what} bytes[{t}]"
    for j, t in enumerate(tags):
        assert got.totals[t] == {"present": int((ty[j] != 0).sum()), "bytes": int(data[t].size) if t in data else 0}, (what, t)


# ---- fixtures --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("split_size", [100 * 1024, 1 << 40])
@pytest.mark.parametrize("name", ["2.bam", "5k.bam"])
def test_fixture_tags(name, split_size, gpu_files, oracle_files):
    o, offs, fields, _, _ = decoded(name, oracle_files)
    g = gpu_files(name)
    _, cols = g.load_records(split_size, columns=("offset",))
    assert cols["offset"].tolist() == offs
    got = g.load_record_tags(QUERY18, bytes_for=QUERY18)
    auxs = [aux_of(fields, k) for k in range(len(offs))]
    assert_tags(got, auxs, QUERY18, QUERY18, what=name)
    assert got.totals["XA"]["present"] == {"2.bam": 1257, "5k.bam": 2004}[name] and got.totals["ZZ"]["present"] == 0
    assert g.kernel_ms("record_tags") > 0
    # rel indexes the record's slice of load_record_fields' aux column: the bytes there are the value
    rf = g.load_record_fields(fields=("aux",))
    assert np.array_equal(rf.aux, fields.aux) and np.array_equal(rf.aux_off, fields.aux_off)
    aux = rf.aux.tobytes()
    for j, t in enumerate(QUERY18):
        texts = got.texts(t)
        for k in np.flatnonzero(got.type[j]).tolist():
            at = int(rf.aux_off[k]) + int(got.rel[j, k])
            assert aux[at - 3:at - 1] == t.encode() and aux[at - 1] == got.type[j, k]
            if chr(got.type[j, k]) in "ZH":
                assert aux[at:at + int(got.value[j, k])] == texts[k] and aux[at + len(texts[k])] == 0


# ---- hand-built records ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def handmade_tags(oracle_files):
    """2.bam's stream with hand-built records inserted after its record 800 and one appended at its end: every list of
    hand_lists() and big_lists() (test_record_tags_host.py) on records whose names of 1..8 bytes put their starts at
    all four residues mod 4, and a 400 000-base record with tags between 1-base records.  The appended record's last
    tag ends at the stream's last byte."""
    o, offs, _, _, _ = decoded("2.bam", oracle_files)
    u = o.u[:o.L].tobytes()
    at = offs[800]
    rng = np.random.default_rng(20261019)
    recs = []
    for i, (_, aux) in enumerate(hand_lists() + big_lists()):
        recs.append(_rand_record(rng, b"abcdefgh"[:1 + i % 8], 1 + i % 3, aux))
    recs.append(_rand_record(rng, b"uv", 1, b"NMC\x11"))
    recs.append(record(b"big", [(400000 << 4) | 0], rng.integers(0, 256, 200000, dtype=np.uint8).tobytes(),
                       rng.integers(0, 64, 400000, dtype=np.uint8).tobytes(), 400000,
                       b"ASC\x21" + b"RGZgrp1\0" + b"NMs\x34\x12"))
    recs.append(_rand_record(rng, b"uvwxyz", 1, b"NMC\x12"))
    last = _rand_record(rng, b"last", 9, b"RGZtail\0" + b"NMi" + struct.pack("<i", -5))
    u2 = u[:at] + b"".join(recs) + u[at:] + last
    arr = np.frombuffer(u2, np.uint8)
    chain = record_chain(arr, int(o.header_end), len(u2))
    assert len(chain) == len(offs) + len(recs) + 1
    starts = np.array(chain[800:800 + len(recs)])
    assert set((starts % 4).tolist()) == {0, 1, 2, 3}
    fields = ref_fields(arr, chain)
    auxs = [aux_of(fields, k) for k in range(len(chain))]
    assert auxs[-1].endswith(b"NMi" + struct.pack("<i", -5)) and chain[-1] + len(last) == len(u2)
    sizes = np.diff(np.array(chain + [len(u2)]))
    assert (sizes > 65536).sum() == 3, "the two big values and the big record span more than one BGZF block"
    lens = [len(a) for a in auxs]
    assert {LONG - 1, LONG, LONG + 1} <= set(lens) and max(lens) > 200000
    return bgzf(u2), arr, chain, auxs


@gpu
class TestHandBuilt:
    @pytest.fixture(scope="class")
    def g(self, handmade_tags):
        import sbam
        blob, u, chain, auxs = handmade_tags
        assert sbam.load_library().sbam_tag_long_aux_bytes() == LONG
        f = sbam.BamFile(blob, path="handmade_tags.bam")
        assert f.uncompressed_size == u.size
        _, cols = f.load_records(1 << 40, columns=("offset",))
        assert cols["offset"].tolist() == chain
        yield f
        f.close()

    def test_all_columns(self, g, handmade_tags):
        blob, u, chain, auxs = handmade_tags
        got = g.load_record_tags(HAND_QUERY, bytes_for=HAND_QUERY)
        assert_tags(got, auxs, HAND_QUERY, HAND_QUERY, what="handmade")
        # the two accessors, on the every-type record
        k = 800 + [label for label, _ in hand_lists()].index("every type")
        f = got.floats("Xf")[k], got.floats("Xg")[k], got.floats("Xh")[k]
        assert f[0] == 0 and np.signbit(f[0]) and np.isnan(f[1]) and f[2] == np.float32(1e10)
        assert got.texts("XH")[k] == b"1AE301" and got.texts("XE")[k] == b"" and got.texts("XH")[0] is None

    def test_the_inserted_run_and_the_last_record_alone(self, g, handmade_tags):
        blob, u, chain, auxs = handmade_tags
        n_ins = len(chain) - 2500 - 1
        q, b = ["NM", "MD", "ZB", "RG"], ["MD", "ZB", "RG"]
        assert_tags(g.load_record_tags(q, 800, n_ins, bytes_for=b), auxs[800:800 + n_ins], q, b, what="inserted")
        assert_tags(g.load_record_tags(q, len(chain) - 1, 1, bytes_for=b), auxs[-1:], q, b, what="last")


# ---- batches, query sizes, byte-column subsets, coexistence ----------------------------------------------------------
@pytest.fixture(scope="module")
def g2(gpu_files, oracle_files):
    o, offs, fields, _, _ = decoded("2.bam", oracle_files)
    g = gpu_files("2.bam")
    g.load_records(1 << 40, columns=None)
    return g, [aux_of(fields, k) for k in range(len(offs))], fields


@gpu
@pytest.mark.parametrize("i0,n", [(0, 0), (7, 0), (0, 1), (2499, 1), (311, 977)])
def test_batches(i0, n, g2):
    g, auxs, _ = g2
    got = g.load_record_tags(QUERY18, i0, n, bytes_for=QUERY18)
    assert (got.i0, got.n) == (i0, n)
    assert_tags(got, auxs[i0:i0 + n], QUERY18, QUERY18, what=f"[{i0}, {i0 + n})")
    if n == 0:
        assert all(v == {"present": 0, "bytes": 0} for v in got.totals.values())
        assert all(o.tolist() == [0] for o in got.bytes_off.values())


def _same(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("type", "sub", "rel", "value")) and \
        all(np.array_equal(a.bytes_off[t], b.bytes_off[t]) and np.array_equal(a.bytes[t], b.bytes[t]) for t in a.bytes)


@gpu
def test_consecutive_batches_make_the_whole_and_repeat_exactly(g2):
    g, auxs, _ = g2
    q, by = ["NM", "RG", "MD", "XA"], ["RG", "MD", "XA"]
    a, b = g.load_record_tags(q, 0, 1111, bytes_for=by), g.load_record_tags(q, 1111, None, bytes_for=by)
    whole = want_columns(auxs, q, by)
    for i, k in enumerate(("type", "sub", "rel", "value")):
        assert np.array_equal(np.concatenate([getattr(a, k), getattr(b, k)], axis=1), whole[i]), k
    for t in by:
        assert np.array_equal(np.concatenate([a.bytes_off[t], b.bytes_off[t][1:] + a.bytes_off[t][-1]]), whole[4][t]), t
        assert np.array_equal(np.concatenate([a.bytes[t], b.bytes[t]]), whole[5][t]), t
    g.load_record_tags(QUERY18, bytes_for=QUERY18)  # a larger batch and query use the buffers in between
    again = g.load_record_tags(q, 1111, None, bytes_for=by)
    assert _same(again, b) and _same(g.load_record_tags(q, 1111, None, bytes_for=by), again)


@gpu
def test_one_tag_and_thirty_two_tags_and_byte_subsets(g2):
    import sbam
    g, auxs, _ = g2
    assert_tags(g.load_record_tags(["NM"]), auxs, ["NM"], [], what="1 tag")
    q32 = QUERY18[:17] + ["Z%d" % i for i in range(10)] + ["Za", "Zb", "Zc", "Zd", "ZZ"]
    assert len(q32) == 32 == sbam.MAX_TAGS
    by = ["MD", "ZZ", "XA", "Z3"]
    got = g.load_record_tags(q32, 5, 2001, bytes_for=by)
    assert_tags(got, auxs[5:2006], q32, by, what="32 tags")
    # the device side: byte columns only for the entries that asked; the host side refuses the others
    dev, i0, n, nq = sbam._RecordTags(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
    assert g.L.sbam_record_tags_device(g.ctx, ctypes.byref(dev), ctypes.byref(i0), ctypes.byref(n),
                                       ctypes.byref(nq)) == sbam.SBAM_OK
    assert (i0.value, n.value, nq.value) == (5, 2001, 32) and dev.type and dev.sub and dev.rel and dev.value
    for j, t in enumerate(q32):
        assert bool(dev.bytes_off[j]) == bool(dev.bytes[j]) == (t in by), t
    buf = np.zeros(1 << 20, np.uint8)
    ask = sbam._RecordTags()
    ask.bytes[q32.index("NM")] = buf.ctypes.data
    assert g.L.sbam_get_record_tags(g.ctx, ctypes.byref(ask)) == sbam.ERR_ARG
    ask = sbam._RecordTags()
    ask.bytes_off[q32.index("MD")] = buf.ctypes.data
    assert g.L.sbam_get_record_tags(g.ctx, ctypes.byref(ask)) == sbam.SBAM_OK
    assert np.array_equal(buf[:8 * 2002].view(np.int64), got.bytes_off["MD"])
    dev_only = g.load_record_tags(q32, 5, 2001, bytes_for=by, host=False)
    assert dev_only.type is None and dev_only.bytes is None and dev_only.totals == got.totals


@gpu
def test_fields_and_tags_coexist(g2):
    import sbam
    g, auxs, fields = g2
    q = ["NM", "RG"]

    def device_names():
        dev = sbam._RecordFields()
        assert g.L.sbam_record_fields_device(g.ctx, ctypes.byref(dev), None, None) == sbam.SBAM_OK
        return dev

    rf = g.load_record_fields(100, 900, fields=("name", "aux"))
    rt = g.load_record_tags(q, 100, 900, bytes_for=["RG"])
    name, aux = np.zeros(rf.name.size, np.uint8), np.zeros(rf.aux.size, np.uint8)
    ask = sbam._RecordFields(name=name.ctypes.data, aux=aux.ctypes.data)
    assert g.L.sbam_get_record_fields(g.ctx, ctypes.byref(ask)) == sbam.SBAM_OK and device_names().name
    assert np.array_equal(name, rf.name) and np.array_equal(aux, rf.aux)
    # the other order: the tags stay readable after a later load_record_fields
    g.load_record_fields(0, 2500)
    back = sbam.RecordTags(100, 900, tuple(q), rt.totals, np.zeros_like(rt.type), np.zeros_like(rt.sub),
                           np.zeros_like(rt.rel), np.zeros_like(rt.value), {"RG": np.zeros_like(rt.bytes_off["RG"])},
                           {"RG": np.zeros_like(rt.bytes["RG"])})
    ask = sbam._RecordTags(type=back.type.ctypes.data, sub=back.sub.ctypes.data, rel=back.rel.ctypes.data,
                           value=back.value.ctypes.data)
    ask.bytes_off[1], ask.bytes[1] = back.bytes_off["RG"].ctypes.data, back.bytes["RG"].ctypes.data
    assert g.L.sbam_get_record_tags(g.ctx, ctypes.byref(ask)) == sbam.SBAM_OK
    assert _same(back, rt)
    assert_tags(back, auxs[100:1000], q, ["RG"], what="after load_record_fields")


# ---- errors ----------------------------------------------------------------------------------------------------------
@gpu
def test_state_and_argument_errors():
    import sbam
    tot = sbam._RecordTagTotals()

    def query(*tags):
        q = (sbam._TagQuery * max(len(tags), 1))()
        for j, t in enumerate(tags):
            q[j].tag = t
        return q

    with sbam.BamFile(fixture_bytes("2.bam"), path="2.bam") as g:
        L = g.L
        call = lambda i0, n, q, nq: L.sbam_load_record_tags(g.ctx, i0, n, q, nq, ctypes.byref(tot))  # noqa: E731
        nm = query(b"NM")
        assert call(0, 1, nm, 1) == sbam.ERR_STATE
        assert L.sbam_record_tags_device(g.ctx, ctypes.byref(sbam._RecordTags()), None, None, None) == sbam.ERR_STATE
        assert L.sbam_get_record_tags(g.ctx, ctypes.byref(sbam._RecordTags())) == sbam.ERR_STATE
        g.load_records(1 << 40, columns=None)
        n_nm = sum(r[1 + QUERY18.index("NM")] != "*" for r in golden_table("2"))
        assert call(0, 2500, nm, 1) == sbam.SBAM_OK and tot.present[0] == n_nm > 2000
        for i0, n in ((0, 2501), (2500, 1), (-1, 1), (0, -1)):
            assert call(i0, n, nm, 1) == sbam.ERR_ARG
        assert call(0, 1, nm, 0) == sbam.ERR_ARG and call(0, 1, query(*[b"NM"] * 33), 33) == sbam.ERR_ARG
        assert call(0, 1, None, 1) == sbam.ERR_ARG
        for bad in (b"1M", b"N_", b"N ", b"\0\0", b"_M", b"N\xe9"):
            assert call(0, 1, query(bad), 1) == sbam.ERR_ARG, bad
        for ok in (b"N0", b"zz", b"Z9", b"aB"):
            assert call(0, 1, query(ok), 1) == sbam.SBAM_OK, ok
        assert call(0, 1, query(b"NM", b"RG", b"NM"), 3) == sbam.ERR_ARG
        assert call(2500, 0, nm, 1) == sbam.SBAM_OK and tot.present[0] == 0
        with pytest.raises(ValueError):
            g.load_record_tags(["NMX"])
        with pytest.raises(ValueError):
            g.load_record_tags(["NM"], bytes_for=["RG"])
        assert call(0, 1, nm, 1) == sbam.SBAM_OK
        g.reset()
        assert call(0, 1, nm, 1) == sbam.ERR_STATE
        g.run()
        g.load_records(1 << 40, columns=None)
        assert call(0, 1, nm, 1) == sbam.SBAM_OK
        g.load_records(1 << 40, columns=None)  # a new load drops the tags
        assert L.sbam_get_record_tags(g.ctx, ctypes.byref(sbam._RecordTags())) == sbam.ERR_STATE


@pytest.fixture(scope="module")
def short_stream(oracle_files):
    """2.bam's header and first 40 records: the base of the malformed files."""
    o, offs, _, _, _ = decoded("2.bam", oracle_files)
    return o.u[:offs[40]].tobytes(), offs[:40]


@gpu
@pytest.mark.parametrize("label,aux", malformed_lists(), ids=[k for k, _ in malformed_lists()])
def test_malformed_tag_lists(label, aux, short_stream):
    """One file per malformed kind: two bad records with good ones between; load_records with one split walks the
    chain by block_size, so it lists them; the tags call reports the first one's offset and produces nothing; batches
    that exclude the bad records succeed, and so does a good call after the error."""
    import sbam
    u, offs = short_stream
    rng = np.random.default_rng(7)
    good = [_rand_record(rng, b"g%d" % i, 3, b"NMC\x05" + b"RGZgrp\0") for i in range(3)]
    bad = _rand_record(rng, b"bad", 2, aux)
    u2 = u + good[0] + bad + good[1] + bad + good[2]
    x_bad = len(u) + len(good[0])
    with sbam.BamFile(bgzf(u2), path="malformed.bam") as g:
        _, cols = g.load_records(1 << 40, columns=("offset",))
        assert cols["offset"].tolist() == offs + [len(u), x_bad, x_bad + len(bad), x_bad + len(bad) + len(good[1]),
                                                  x_bad + 2 * len(bad) + len(good[1])]
        with pytest.raises(sbam.RecordFieldsException) as ei:
            g.load_record_tags(["ZZ"])
        assert ei.value.position == x_bad
        e = g.L.sbam_last_error(g.ctx).contents
        assert e.code == sbam.ERR_RECORD and e.position == x_bad
        assert g.L.sbam_record_tags_device(g.ctx, ctypes.byref(sbam._RecordTags()), None, None, None) == sbam.ERR_STATE
        with pytest.raises(sbam.RecordFieldsException) as ei:
            g.load_record_tags(["NM"], 42, 3)
        assert ei.value.position == x_bad + len(bad) + len(good[1])
        before = g.load_record_tags(["NM", "RG"], 0, 41, bytes_for=["RG"])
        assert before.value[0, 40] == 5 and before.texts("RG")[40] == b"grp"
        assert g.load_record_tags(["NM"], 42, 1).value[0, 0] == 5
        assert g.load_record_fields(41, 1, fields=("aux",)).aux.tobytes() == aux  # (the fields do not parse tags)


@gpu
def test_structural_failures_are_reported_the_same_way(oracle_files):
    import sbam
    o, offs, _, _, _ = decoded("2.bam", oracle_files)
    u = bytearray(o.u[:o.L].tobytes())
    struct.pack_into("<i", u, offs[1200] + 20, 100000)  # l_seq claims more than block_size holds
    struct.pack_into("<i", u, offs[1300] + 20, -1)
    with sbam.BamFile(bgzf(bytes(u)), path="overrun.bam") as g:
        g.load_records(1 << 40, columns=None)
        with pytest.raises(sbam.RecordFieldsException) as ei:
            g.load_record_tags(["NM"])
        assert ei.value.position == offs[1200]
        with pytest.raises(sbam.RecordFieldsException) as ei:
            g.load_record_tags(["NM"], 1201, 200)
        assert ei.value.position == offs[1300]
        n_nm = sum(r[1 + QUERY18.index("NM")] != "*" for r in golden_table("2")[:1200])
        assert g.load_record_tags(["NM"], 0, 1200).totals["NM"]["present"] == n_nm > 1000


# ---- CLI -------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["2", "5k"])
def test_cli_tags_equals_the_reference_sam(name, tmp_path):
    from sbam import cli
    out = tmp_path / "tags.tsv"
    assert cli.main(["tags", "-t", ",".join(QUERY18), "-m", "100k", "--verify-crc",
                     os.path.join(FIXTURES, name + ".bam"), str(out)]) == 0
    got = [ln.split("\t") for ln in out.read_text(encoding="latin-1").split("\n")]
    assert got.pop() == [""] and got == golden_table(name)


# ---- the synthetic file ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("read_len", [150, 0])
def test_synthetic(read_len):
    import oracle
    import sbam
    import synth
    s = synth.SynthBam(tile_mb=4, copies=1, read_len=read_len, threads=8)
    d = s.bytes()
    o = oracle.BamFile(d, threads=8)
    _, _, first = stream_header(o.u)
    chain = record_chain(o.u, first, o.L)
    assert len(chain) == s.n_records
    fields = ref_fields(o.u[:o.L], chain)
    auxs = [aux_of(fields, k) for k in range(len(chain))]
    q, by = ["NM", "AS", "XS", "RG", "MD"], ["RG", "MD"]
    with sbam.BamFile(d, path="synth.bam") as g:
        g.load_records(256 * 1024, columns=None)
        got = g.load_record_tags(q, bytes_for=by)
        assert_tags(got, auxs, q, by, what=f"synthetic, read_len {read_len}")
        assert got.totals["RG"]["present"] > 0 and got.totals["RG"]["bytes"] > 0
