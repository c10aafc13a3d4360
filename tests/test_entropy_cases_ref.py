"""The crafted planes of tests/entropy_cases.py on the CPU: the model of the coder equals the reference, the oracle's restatement equals
the reference, every case exercises what its labels say, and the cases together cover what the GPU module is there to reach.

The conditions every case meets on the reference (asserted, not tolerances): its section is at most half of the buffer the plane
tests hand over, shorter than cw * ch * 8 bytes -- the reference's decoder refuses anything longer (hzcc.c:627) --, and the reference
decodes it back to the plane it was made from."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import dsvabi as A
import entropy_cases as E
from entropy_cases import CASES

pytestmark = pytest.mark.skipif(not os.path.exists(A.REF_SO), reason="oracle/_ref not built")


@functools.lru_cache(maxsize=None)
def reference_section(case, plane=0, offset=0):
    """(buffer, bs.pos) of the reference's dsv_encode_plane, the three conditions asserted; computed once, shared, read-only"""
    ref = A.load_ref()
    buf, pos, coefs = E.encode_plane(ref, case, plane, offset)
    nbytes = pos // 8 - offset
    assert pos % 8 == 0 and pos // 8 <= len(buf) // 2, "the section outgrew half of its buffer"
    assert nbytes < case.w * case.h * 8, "the reference's decoder would refuse the section (hzcc.c:627)"
    assert np.array_equal(coefs, case.plane()), "lossless: the coefficients stay as they are"
    ok, dpos, back = E.decode_plane(ref, buf, case, plane, offset)
    assert ok == 1 and dpos == pos and np.array_equal(back, case.plane()), "the reference does not decode its own section"
    buf.setflags(write=False)
    return buf, pos


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_model_gives_the_reference_section_length(case):
    buf, pos = reference_section(case)
    m = case.model()
    assert pos // 8 == m.section_bytes
    assert int.from_bytes(bytes(buf[:4]), "big") == m.section_bytes - 4


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_oracle_equals_reference(case):
    buf, pos = reference_section(case)
    orc = A.load_oracle()
    coefs = np.array(case.plane())
    out = np.zeros(E.buffer_bytes(case), dtype=np.uint8)
    fm, (meta, params, bd, mvs) = E._fmeta(case, 0)
    n = orc.orc_encode_plane(A.np_ptr(out, C.c_uint8), 0, A.np_ptr(coefs, C.c_int32), case.w, case.h, 1, 0, 0, 1, params.do_psy, 0, 0,
                             params.blk_w, params.blk_h, params.nblocks_h, params.nblocks_v, A.np_ptr(bd, C.c_uint8), C.c_void_p(mvs.ctypes.data))
    assert n == pos // 8 and np.array_equal(out[:n], buf[:n])
    assert np.array_equal(coefs, case.plane())


@pytest.mark.parametrize("plane", [1, 2])
@pytest.mark.parametrize("name", E.GEOMETRY_CASES)
def test_reference_section_does_not_depend_on_the_plane_index(name, plane):
    case = E.BY_NAME[name]
    buf, pos = reference_section(case, plane)
    buf0, pos0 = reference_section(case)
    assert pos == pos0 and np.array_equal(buf[:pos // 8], buf0[:pos // 8])


@pytest.mark.parametrize("offset", E.OFFSETS[1:])
@pytest.mark.parametrize("name", E.OFFSET_CASES)
def test_reference_section_moves_with_its_offset(name, offset):
    case = E.BY_NAME[name]
    buf, pos = reference_section(case, 0, offset)
    buf0, pos0 = reference_section(case)
    assert pos == pos0 + 8 * offset and np.array_equal(buf[offset:pos // 8], buf0[:pos0 // 8]) and np.all(buf[:offset] == E.LEAD)


# ---- the labels ---------------------------------------------------------------------------------------------------------------------
def _check(kind, want, m):
    if kind == "flags":
        assert m.flags() == want
    elif kind == "n":
        assert m.n == want
    elif kind == "nskip":
        assert m.nskip == want
    elif kind == "nch":
        assert m.nch == want
    elif kind == "min_nch":
        assert m.nch >= want
    elif kind == "chunk_start":
        for c, st in want.items():
            assert m.chunk_start[c] == st, "state at the start of chunk %d" % c
    elif kind == "end_state":
        assert m.chain_states()[-1] == want
    elif kind == "peak":
        assert int(m.met.max()) == want
    elif kind == "join":
        for c, tl in want.items():
            assert m.join(c) == tl, "chunk %d: (symbols to the join, the look that sees it)" % c
    elif kind == "hands_on":
        # the chunk is a test of the join only through the state it hands on, and only where a wrong join hands on another one
        for c, wrong in want.items():
            true = int(m.met[(c + 1) * E.CHUNK])
            assert m.nch > c + 1 and m.handover(c) == true, "chunk %d: the kernels' way to the state behind it" % c
            assert (m.handover(c, swap=True) != true) == ("swap" in wrong), "chunk %d: the pair's end states swapped" % c
            assert (m.handover(c, join_range=2) != true) == ("range2" in wrong), "chunk %d: joined at a range of 2" % c
    elif kind == "chunk_value_bits":
        for c, bits in want.items():
            assert int(m.val_len[c * E.CHUNK:(c + 1) * E.CHUNK].sum()) == bits
    elif kind == "value_bits":
        assert m.value_bits == want
    elif kind == "min_bytes":
        assert m.section_bytes >= want
    elif kind == "val_len":
        for i, bits in want.items():
            assert m.val_len[i] == bits
    elif kind == "run_len":
        for i, bits in want.items():
            assert m.run_len[i] == bits
    elif kind == "val_run_len":
        for i, bits in want.items():
            assert m.val_len[i] + m.run_len[i + 1] == bits
    elif kind == "flips":
        for level, least in want.items():
            assert m.longest_flip_run(level) >= least, "symbols of level %d whose k differs from their predecessor's" % level
    elif kind == "tail":
        assert m.codes_in_tail(256) >= want
    elif kind == "straddle":
        assert m.straddles() >= want
    else:
        raise AssertionError("no such label: " + kind)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_labels_hold_in_the_model(case):
    m = case.model()
    assert "flags" in case.labels
    for kind, want in case.labels.items():
        _check(kind, want, m)
    assert np.all(np.abs(m.val) <= E.VMAX) and abs(m.ll) <= E.VMAX


def test_cases_cover_every_label():
    models = {c.name: c.model() for c in CASES}
    kinds = set(k for c in CASES for k in c.labels)
    assert kinds >= {"flags", "n", "nskip", "nch", "min_nch", "chunk_start", "end_state", "peak", "join", "hands_on", "chunk_value_bits", "value_bits", "min_bytes", "val_len",
                     "run_len", "val_run_len", "flips", "tail", "straddle"}
    # each of flags 1, 4 and 8 expected by one case and not by a neighbour of the same kind
    flags = {n: m.flags() for n, m in models.items()}
    assert flags["dense-65-finest"] == 1 and flags["dense-64-finest"] == 0
    assert flags["dense-128-shift2"] == 1 and flags["dense-128-shift1"] == 0
    assert flags["dense-128-end256"] == 1 and flags["dense-128-end255"] == 0
    assert flags["dense-16385-level1"] == 1 and flags["dense-16384-level1"] == 0
    assert flags["absurd-chunk-640x480"] == 4 and flags["over-mirror-640x480"] == 8 and flags["run-max-640x480"] == 0
    assert not any(f & 2 for f in flags.values())  # (out of reach: entropy_cases.py says why)
    # where the 256 trajectories stand: never joined over a full chunk, joined at the first look, one symbol either side of a look,
    # behind the last look, a chunk too short for a look
    joins = [models[n].join(c) for n, c in (("alt-3000-m1", 0), ("alt-129-m1-from-255", 1), ("join-at-first-look", 1), ("join-one-before-look", 1),
                                            ("join-one-after-look", 1), ("join-in-last-64", 1), ("short-rice-chunk", 0))]
    assert joins == [(None, None), (None, None), (128, 128), (127, 128), (129, 192), (995, None), (None, None)]
    assert int(np.count_nonzero(models["short-rice-chunk"].seg[:E.CHUNK])) == 74
    # every join chunk hands its state to a chunk behind it; behind the chunks of the 5-symbol family every code hangs on that state's
    # parity (k changes with each symbol for more than 900 of the 1024); a swapped pair and a join at a range of 2 each hand on
    # another state for a named case
    wrong = [w for c in CASES for w in c.labels.get("hands_on", {}).values()]
    assert len(wrong) == 8 and sum("swap" in w for w in wrong) == 4 and sum("range2" in w for w in wrong) == 1
    for n in ("join-at-first-look", "join-one-before-look", "join-one-after-look", "laplace-one-chunk"):
        k = models[n].k[2 * E.CHUNK:]
        assert int(np.count_nonzero(k[1:] != k[:-1])) > 900
    # chunk counts either side of k_ent_chain's batch of 32 and of a wavefront of 64 lanes, symbol counts round a chunk's end
    assert sorted(m.n for m in models.values() if m.n <= 2048)[:2] == [0, 1]
    assert {0, 1, 1023, 1024, 1025, 2048} <= {m.n for m in models.values()}
    assert any(32 < m.nch <= 64 for m in models.values()) and any(m.nch > 64 for m in models.values())
    # LL prefixes: every residue of 4, 15 and 0 of 16, a whole chunk, more than a chunk, the whole plane
    skips = {m.nskip for m in models.values()}
    assert {15, 16, 17, 18, 19, 1024, 1100} <= skips and any(m.nskip == m.n > 0 for m in models.values())
    # the parser's lane rules: value codes of 40 and 41 bits, value + run of 64 and 65, runs of 1, 31 and the most a 640 x 480 plane has
    lens = lambda kind: sorted(b for c in CASES for b in c.labels.get(kind, {}).values())  # noqa: E731
    assert lens("val_len") == [40, 41, 60000] and lens("val_run_len") == [64, 65] and lens("run_len") == [1, 25, 31, 37]
    for level in range(3):
        assert max(m.longest_flip_run(level) for m in models.values()) >= 150
    assert models["floor-0"].met.max() == 0 and models["floor-0"].n >= 2000


# ---- a real picture inside the packet bound that reaches flag 1 -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream_reference(which):
    import stream_sections as S
    return S.reference_of(S.flag1_stream() if which == "flag1" else S.neighbour_stream())


def test_checkerboard_stream_reaches_flag_1_inside_the_packet_bound():
    import stream_sections as S
    from edge_cases import packet_bound_holds
    pk, _, flagged = stream_reference("flag1")
    packet_bound_holds(pk, S.FLAG1_W, S.FLAG1_H, A.SUBSAMP_420)
    assert [p[5] & 5 for p in pk[1:]] == [4, 5], "an I and a P picture"
    models = S.plane_models(pk[1], S.FLAG1_W, S.FLAG1_H, A.SUBSAMP_420)
    print("I picture of %d bytes; states behind the chunks reach %s" % (len(pk[1]), [max(m.chain_states()) for m in models]))
    assert [m.flags() & 1 for m in models] == [1, 1, 1] and flagged == 1
    assert all(m.n == 0 for m in S.plane_models(pk[2], S.FLAG1_W, S.FLAG1_H, A.SUBSAMP_420)), "the P picture of a still: no symbol"
    npk, _, nflagged = stream_reference("neighbour")
    packet_bound_holds(npk, S.FLAG1_W, S.FLAG1_H, A.SUBSAMP_420)
    assert nflagged == 0 and S.plane_models(npk[1], S.FLAG1_W, S.FLAG1_H, A.SUBSAMP_420)[0].nch > 1, "a neighbour with chunks to chain"


def test_section_parser_reads_back_the_crafted_planes():
    import stream_sections as S
    for name in ("prefix-1100", "dense-256x160", "lone-30000", "flip-k"):
        case = E.BY_NAME[name]
        buf, pos = reference_section(case)
        sv = S.parse_section(bytes(buf[4:pos // 8]), case.scan())
        assert np.array_equal(case.scan().plane_of(sv), case.plane())
