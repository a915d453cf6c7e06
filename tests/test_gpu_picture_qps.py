"""GPU: the pictures of a stacked context at a QP each -- hop_ctx_set_picture_qps, hop_sao_frame_pictures, and hop_access_units_decode over access units whose QPs
differ (csrc/hop_ctx.hip, k_spine.hip, k_entropy.hip, k_parse.hip, k_decode.hip, k_deblock.hip, k_sao.hip, k_stream.hip).

The expected bytes are the unmodified reference encoder's streams of ONE picture at QP 22 / 27 / 32 / 37 (tests/golden/stream_qps.npz, tools/make_golden_qps.py, and the
QP-32 stream of tests/golden/slice_data.npz; the reference switches no SAO flag at any of them, so none had to be moved), shown right on the CPU by
tests/test_picture_qps_cpu.py.  The picture is 192x128, three by two CTUs: two rows, so WaveFrontSynchro's hand-over runs, and three columns, so the row below starts from
the state after the SECOND CTU.  Four pictures put a table index above 1 into every kernel; the four QPs have four different qp % 6 and lie on both sides of the chroma QP
table's knee at 30.  The plain-intra streams (136x72, partial CTUs, 22 / 32 / 37) take the same road without a wavefront."""
import ctypes
import os

import numpy as np
import pytest

import picture_qps_util as Q
import slicedata_util as U
import stream_read_util as R
import stream_util as S

pytestmark = pytest.mark.gpu

KEY = "192x128_wpp"
QPS = list(Q.QPS[KEY])                                                       # 22, 27, 32, 37
C = Q.CASES[KEY]
N = 6                                                                        # CTUs of one picture
WRITE = dict(slice_type=3, wpp=1, plain_intra=0, mi_size=16)
_single, _stack = {}, {}


def planes(ctx):
    return [ctx.recon_download(comp) for comp in range(3)]


def padded(ctx):
    return [ctx.ssref_download(comp) for comp in range(3)]


def single(key, qp):
    """the stream through hop_access_unit_decode on a context of its own: info, parts, levels, sao, planes, padded SS planes; once per stream"""
    if (key, qp) not in _single:
        hp = R.hophip()
        c = Q.CASES[key]
        ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"])
        info, match, parts, levels, sao = ctx.access_unit_decode(Q.stream(key, qp))
        assert match == [1, 1, 1], (key, qp, match)
        _single[(key, qp)] = dict(info=info, parts=parts.copy(), levels=levels.copy(), sao=sao.copy(), planes=planes(ctx), ss=padded(ctx))
        ctx.close()
    return _single[(key, qp)]


def check_planes(ctx, want, what, ss=True):
    """every picture of the stack against the planes (and the padded SS reference, its own margins included) of the single decodes"""
    got = planes(ctx)
    for comp in range(3):
        for k, a in enumerate(ctx.unstack(got[comp], comp > 0)):
            assert np.array_equal(a, want[k]["planes"][comp]), (what, "picture", k, "plane", comp, np.argwhere(a != want[k]["planes"][comp])[:4])
    if not ss:
        return
    s = padded(ctx)
    for k in range(ctx.pictures):
        for comp, (sh, m) in enumerate(((0, 80), (1, 40), (1, 40))):
            a = s[comp][(k * ctx.pitch >> sh):(k * ctx.pitch >> sh) + (ctx.sub_h >> sh) + 2 * m]
            assert np.array_equal(a, want[k]["ss"][comp]), (what, "SS reference of picture", k, comp, np.argwhere(a != want[k]["ss"][comp])[:4])


def decoded_stack(key):
    """ONE hop_access_units_decode of the case's streams, one per QP, into a stack: (infos, match, parts, levels, sao); checked by test_decode_*, shared by the rest"""
    if key not in _stack:
        hp = R.hophip()
        c, qps = Q.CASES[key], Q.QPS[key]
        ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"], pictures=len(qps))     # no original, no table
        infos, match, parts, levels, sao = ctx.access_units_decode([Q.stream(key, qp) for qp in qps])
        _stack[key] = dict(infos=infos, match=match, parts=parts.copy(), levels=levels.copy(), sao=sao.copy(), ctx=ctx)
    return _stack[key]


@pytest.mark.parametrize("key", list(Q.QPS))
def test_decode_streams_of_different_qps_in_one_call(key):
    c, qps = Q.CASES[key], Q.QPS[key]
    n = ((c["W"] + 63) // 64) * ((c["H"] + 63) // 64)
    d = decoded_stack(key)
    want = [single(key, qp) for qp in qps]
    assert d["match"] == [[1, 1, 1]] * len(qps), d["match"]                   # the reference encoder's own MD5 of every picture
    for k, (qp, w) in enumerate(zip(qps, want)):
        assert d["infos"][k].params.slice.qp == qp and bytes(d["infos"][k]) == bytes(w["info"]), (key, k)
        assert d["parts"][k * n:(k + 1) * n].tobytes() == w["parts"].tobytes(), (key, "parts", k)
        assert np.array_equal(d["levels"][k * n:(k + 1) * n], w["levels"]), (key, "levels", k)
        assert d["sao"][k * n:(k + 1) * n].tobytes() == w["sao"].tobytes(), (key, "sao", k)
    check_planes(d["ctx"], want, key, ss=not c["plain"])


def test_decode_ignores_the_table_and_still_refuses_other_fields():
    hp = R.hophip()
    want = [single(KEY, qp) for qp in (37, 22)]
    ctx = hp.Context(192, 128, pictures=2)
    ctx.set_picture_qps([30, 30])                                            # neither read nor changed: every picture at the QP of its own stream
    infos, match = ctx.access_units_decode([Q.stream(KEY, 37), Q.stream(KEY, 22)], want_outputs=False)[:2]
    assert match == [[1, 1, 1]] * 2 and [i.params.slice.qp for i in infos] == [37, 22]
    check_planes(ctx, want, "table set")
    before = planes(ctx)
    with pytest.raises(hp.HopError) as e:                                    # the micro-image sizes differ (and the QPs)
        ctx.access_units_decode([Q.stream(KEY, 22), U.load_fixture()["192x128_seed7_mi15_wpp/bin"].tobytes()], want_outputs=False)
    assert e.value.code == -1 and "access unit 1" in str(e.value) and "mi_size" in str(e.value), e.value
    with pytest.raises(hp.HopError) as e:                                    # the SAO flags differ
        ctx.access_units_decode([Q.stream(KEY, 22), U.load_fixture()["192x128_wpp_sao0/bin"].tobytes()], want_outputs=False)
    assert e.value.code == -1 and "access unit 1" in str(e.value) and "SAO" in str(e.value), e.value
    assert all(np.array_equal(a, b) for a, b in zip(before, planes(ctx)))
    ctx.close()
    one = hp.Context(192, 128)                                               # hop_access_unit_decode: the stream's QP, whatever the table says
    one.set_picture_qps([40])
    assert one.access_unit_decode(Q.stream(KEY, 22), want_outputs=False)[1] == [1, 1, 1]
    one.close()


def reference_slice_data(key, qps):
    """per QP (the slice data of the reference stream as RBSP, its substream sizes): hop_access_unit_read_host"""
    out = [R.hophip().access_unit_read_host(Q.stream(key, qp), None) for qp in qps]
    return [o[1] for o in out], [o[2] for o in out]


@pytest.mark.parametrize("key", list(Q.QPS))
def test_picture_level_kernels_follow_the_table(key):
    """no encode: from the parts and levels of the decode above, with the table set and qp=32 in every call's params -- decode, deblock, SAO; slice data written and parsed
    back; whole access units.  Then the table cleared: the same write gives the QP-32 picture's bytes alone."""
    hp = R.hophip()
    c, qps = Q.CASES[key], list(Q.QPS[key])
    n = ((c["W"] + 63) // 64) * ((c["H"] + 63) // 64)
    plain = 1 if c["plain"] else 0
    d = decoded_stack(key)
    want = [single(key, qp) for qp in qps]
    args = dict(slice_type=c["slice_type"], wpp=c["wpp"], plain_intra=plain, mi_size=c["mi"])
    ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"], pictures=len(qps))
    ctx.set_picture_qps(qps)
    ctx.decode_stack(d["parts"], d["levels"], qp=32, plain_intra=plain)
    ctx.deblock_frame(d["parts"], 32)
    recon = np.concatenate([hp.sao_reconstruct_params(d["sao"][k * n:(k + 1) * n], (c["W"] + 63) // 64, c["bd"]) for k in range(len(qps))])
    ctx.sao_apply(recon)
    check_planes(ctx, want, key + ": decode_stack, deblock_frame, sao_apply", ss=False)
    # the slice data: every picture's substreams are the reference stream's
    ref_data, ref_sizes = reference_slice_data(key, qps)
    data, sizes, n_sub = ctx.slice_data_write(d["parts"], d["levels"], d["sao"], qp=32, **args)
    rows = c["rows"]
    assert n_sub == rows and len(sizes) == rows * len(qps)
    at = 0
    for k in range(len(qps)):
        mine = int(sizes[k * rows:(k + 1) * rows].sum())
        assert np.array_equal(sizes[k * rows:(k + 1) * rows], ref_sizes[k]) and data[at:at + mine] == ref_data[k], (key, "slice data of picture", k)
        at += mine
    parts, levels, sao = ctx.slice_data_parse(data, sizes, qp=32, sao_luma=1, sao_chroma=1, **args)
    assert parts.tobytes() == d["parts"].tobytes() and np.array_equal(levels, d["levels"]) and sao.tobytes() == d["sao"].tobytes(), key
    # whole access units (the MD5 of the resident pictures in the SEI): the reference encoder's .bin files
    aus, au_sizes = ctx.access_unit_write(d["parts"], d["levels"], d["sao"], qp=32, parameter_sets=1, hash=1, guard=256, **args)
    at = 0
    for k, qp in enumerate(qps):
        got, ref = aus[at:at + int(au_sizes[k])], Q.stream(key, qp)
        assert got == ref, "%s picture %d (QP %d): %s" % (key, k, qp, S.first_difference(got, ref))
        at += int(au_sizes[k])
    # the table cleared: qp=32 for all -- the table, not the params, carried the others
    ctx.set_picture_qps(None)
    aus, au_sizes = ctx.access_unit_write(d["parts"], d["levels"], d["sao"], qp=32, parameter_sets=1, hash=1, **args)
    at = 0
    for k, qp in enumerate(qps):
        assert (aus[at:at + int(au_sizes[k])] == Q.stream(key, qp)) == (qp == 32), (key, k)
        at += int(au_sizes[k])
    ctx.close()


# ---- the encode ----
def code_stack(ctx, qps):
    """the chain of a stack with the table set: (cost, parts, access units per picture)"""
    cost, bits, dist, parts, _ = ctx.encode_frame(32, 16, 0, None, wpp=1, wavefront_lag=5)
    ctx.deblock_frame(parts, 32)
    sao = ctx.sao_frame_pictures([(U.sao_lambdas(qp), 3, qp, 0) for qp in qps])
    data, sizes = ctx.access_unit_write(parts, None, sao, qp=32, parameter_sets=1, hash=1, **WRITE)
    edges = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return cost, parts, [data[edges[k]:edges[k + 1]] for k in range(len(qps))]


def stacked_original(ctx):
    Y, Cb, Cr = C["pictures"][0]
    k = ctx.pictures
    ctx.upload_orig(ctx.stack([Y] * k), ctx.stack([Cb] * k, True), ctx.stack([Cr] * k, True))


def assert_reference_bytes(aus, what):
    for k, qp in enumerate(QPS):
        ref = Q.stream(KEY, qp)
        assert aus[k] == ref, "%s: picture %d (QP %d): %s" % (what, k, qp, S.first_difference(aus[k], ref))


@pytest.fixture(scope="module")
def stack4():
    """the case's original four times in a stack of four, 16 candidate slots, the table set to 22 / 27 / 32 / 37"""
    hp = R.hophip()
    ctx = hp.Context(192, 128, pictures=4, slots=16)
    stacked_original(ctx)
    ctx.set_picture_qps(QPS)
    yield ctx
    ctx.close()


def test_four_rate_points_in_one_wavefront(stack4):
    """hop_encode_frame, hop_deblock_frame, hop_sao_frame_pictures, hop_access_unit_write: the reference encoder's four .bin files byte for byte; per-CTU costs and parts
    of pictures 0 and 3 are those of a context of its own coded at 22 and at 37"""
    hp = R.hophip()
    cost, parts, aus = code_stack(stack4, QPS)
    assert_reference_bytes(aus, "stack of four")
    Y, Cb, Cr = C["pictures"][0]
    for k in (0, 3):
        one = hp.Context(192, 128, slots=16)
        one.upload_orig(Y, Cb, Cr)
        c1, _, _, p1, _ = one.encode_frame(QPS[k], 16, 0, None, wpp=1, wavefront_lag=5)
        one.close()
        assert np.array_equal(cost[k * N:(k + 1) * N], c1), (k, cost[k * N:(k + 1) * N], c1)
        assert parts[k * N:(k + 1) * N].tobytes() == p1.tobytes(), k


def test_picture_groups_code_the_same_bytes(stack4):
    old = os.environ.get("HOP_SPINE_GROUPS")
    os.environ["HOP_SPINE_GROUPS"] = "2"                                     # (read per call) two groups of two pictures on views of the context: they see its table
    try:
        aus = code_stack(stack4, QPS)[2]
    finally:
        if old is None:
            del os.environ["HOP_SPINE_GROUPS"]
        else:
            os.environ["HOP_SPINE_GROUPS"] = old
    assert_reference_bytes(aus, "HOP_SPINE_GROUPS=2")


def test_exact_wavefront_codes_the_same_bytes(stack4):
    stack4.set_exact(True)
    try:
        aus = code_stack(stack4, QPS)[2]
    finally:
        stack4.set_exact(False)
    assert_reference_bytes(aus, "hop_encode_set_exact")


def test_state_and_refusals(stack4):
    hp = R.hophip()
    ctx = stack4

    def refused(fn, *words):
        with pytest.raises(hp.HopError) as e:
            fn()
        assert e.value.code == -1 and all(w in str(e.value) for w in words), (words, e.value)

    cost, parts, aus = code_stack(ctx, QPS)
    # a wrong count, a QP of 52, a NULL table with n > 0: HOP_ERR_ARG, and the table stays (the next chain still writes the four reference streams)
    refused(lambda: ctx.set_picture_qps([22, 27, 32]), "3 QPs", "4 pictures")
    refused(lambda: ctx.set_picture_qps([22, 27, 32, 37, 42]), "5 QPs")
    refused(lambda: ctx.set_picture_qps([22, 27, 52, 37]), "picture 2", "52")
    refused(lambda: ctx.set_picture_qps([22, -1, 32, 37]), "picture 1")
    ctx.L.hop_ctx_set_picture_qps.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    assert ctx.L.hop_ctx_set_picture_qps(ctx.h, 4, None) == -1
    data = ctx.access_unit_write(parts, None, None, qp=32, parameter_sets=1, hash=0, sao_luma=0, sao_chroma=0, **WRITE)[0]
    refused(lambda: ctx.sao_frame(U.sao_lambdas(32), 3, 32, 0), "hop_sao_frame_pictures")
    # disagreeing enabled flags (or slice types): refused with the pictures untouched
    before = planes(ctx)
    lam = [(U.sao_lambdas(qp), 3, qp, 0) for qp in QPS]
    refused(lambda: ctx.sao_frame_pictures(lam[:2] + [lam[2] + ((1, 0, 0),)] + lam[3:]), "hop_sao_frame_pictures", "picture 2", "enabled")
    refused(lambda: ctx.sao_frame_pictures(lam[:3] + [(lam[3][0], 2, 37, 0)]), "hop_sao_frame_pictures", "picture 3", "slice_type")
    assert all(np.array_equal(a, b) for a, b in zip(before, planes(ctx)))
    # the refusals above left the table as it was
    assert ctx.access_unit_write(parts, None, None, qp=32, parameter_sets=1, hash=0, sao_luma=0, sao_chroma=0, **WRITE)[0] == data
    # a table of four equal QPs: the bytes of the plain stacked call
    ctx.set_picture_qps([27] * 4)
    same = ctx.access_unit_write(parts, None, None, qp=32, parameter_sets=1, hash=0, sao_luma=0, sao_chroma=0, **WRITE)[0]
    ctx.set_picture_qps(None)
    plain = ctx.access_unit_write(parts, None, None, qp=27, parameter_sets=1, hash=0, sao_luma=0, sao_chroma=0, **WRITE)[0]
    assert same == plain and same != data
    ctx.sao_frame(U.sao_lambdas(27), 3, 27, 0)                               # (no table: hop_sao_frame decides again)
    ctx.set_picture_qps(QPS)
    # hop_ctx_set_stack clears the table: the picture count changes
    ctx._chk(ctx.L.hop_ctx_set_stack(ctx.h, ctx.sub_h, ctx.pitch), "hop_ctx_set_stack")
    assert ctx.access_unit_write(parts, None, None, qp=27, parameter_sets=1, hash=0, sao_luma=0, sao_chroma=0, **WRITE)[0] == plain
    ctx.set_picture_qps(QPS)                                                 # (as the fixture made it)
    # an unstacked context: n is 1
    one = hp.Context(64, 64)
    refused(lambda: one.set_picture_qps([22, 27]), "2 QPs", "1 picture")
    one.set_picture_qps([22])
    one.set_picture_qps([])
    one.close()
