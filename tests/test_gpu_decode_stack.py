"""GPU: hop_decode_stack, hop_access_units_decode -- the pictures of a stacked context decoded side by side (csrc/k_decode.hip, csrc/k_stream.hip).

Picture k >= 1 is where a wrong origin shows, so every case compares EVERY picture of the stack with a context of its own: the bytes of the unmodified reference
encoder (tests/golden/slice_data.npz) go through hop_access_unit_decode one access unit at a time, and through hop_access_units_decode into a stack; planes, the padded
SS reference with each picture's own margins, parts, levels and SAO parameters must be the same, and every hash the reference wrote must match.  Then the device round
trip of three pictures coded in a stack, hop_decode_stack alone with both schedules, the parser's launch count, and the refusals."""
import numpy as np
import pytest

import slicedata_util as U
import stream_read_util as R
import stream_util as S
from hoputil import lenslet

pytestmark = pytest.mark.gpu

CASES = R.CASES
STACKS = {                                                                  # case -> (fixture key, access unit of that stream) per picture
    "a_two_frames_of_one_sequence": [("128x64_2frames", 0), ("128x64_2frames", 1)],
    "b_two_streams_nxn_and_transform_skip": [("64x64_raster", 0), ("64x64_sharp77", 0)],
    "c_partial_ctus_and_gap_rows": [("200x104_raster", 0)] * 3,
    "d_wavefront_mi15_long_vectors": [("448x192_seed3_mi15_wpp", 0)] * 2,
    "e_plain_10_bit": [("136x72_plain10", 0)] * 2,
}
_single = {}


def access_units(key):
    return R.hophip().annexb_access_units(U.load_fixture()[key + "/bin"].tobytes())


def padded(ctx):
    return [ctx.ssref_download(comp) for comp in range(3)]


def planes(ctx):
    return [ctx.recon_download(comp) for comp in range(3)]


def single(key):
    """every access unit of a fixture stream through hop_access_unit_decode on a context of its own: per access unit (info, parts, levels, sao, planes, padded SS planes);
    computed once per stream"""
    if key not in _single:
        hp = R.hophip()
        c = CASES[key]
        ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"])
        out, active = [], None
        for au in access_units(key):
            info, match, parts, levels, sao = ctx.access_unit_decode(au, active)
            assert match == [1, 1, 1], (key, match)
            out.append(dict(info=info, parts=parts.copy(), levels=levels.copy(), sao=None if sao is None else sao.copy(), planes=planes(ctx), ss=padded(ctx)))
            active = active or info
        ctx.close()
        _single[key] = out
    return _single[key]


def unstacked_ss(ctx, ss):
    """picture k's padded SS planes cut out of the stack's: its own margins above and below"""
    out = []
    for k in range(ctx.pictures):
        out.append([ss[comp][(k * ctx.pitch >> sh):(k * ctx.pitch >> sh) + (ctx.sub_h >> sh) + 2 * m] for comp, (sh, m) in enumerate(((0, 80), (1, 40), (1, 40)))])
    return out


def check_stack_against_singles(ctx, want, plain, what):
    got = planes(ctx)
    for comp in range(3):
        for k, a in enumerate(ctx.unstack(got[comp], comp > 0) if ctx.pictures > 1 else [got[comp]]):
            assert np.array_equal(a, want[k]["planes"][comp]), (what, "picture", k, "plane", comp, np.argwhere(a != want[k]["planes"][comp])[:4])
    if plain:
        return                                                              # an I slice has no SS reference
    ss = padded(ctx)
    for k, three in enumerate(unstacked_ss(ctx, ss) if ctx.pictures > 1 else [ss]):
        for comp in range(3):
            assert np.array_equal(three[comp], want[k]["ss"][comp]), (what, "SS reference of picture", k, comp, np.argwhere(three[comp] != want[k]["ss"][comp])[:4])
    for k in range(ctx.pictures - 1):                                       # the rows between two pictures' margins: the sentinel
        for comp, (sh, m) in enumerate(((0, 80), (1, 40), (1, 40))):
            gap = ss[comp][(k * ctx.pitch >> sh) + (ctx.sub_h >> sh) + 2 * m:(k + 1) * ctx.pitch >> sh]
            assert gap.size and np.all(gap == -1), (what, "gap under picture", k, comp)


@pytest.mark.parametrize("case", sorted(STACKS))
def test_reference_streams_into_a_stack(case):
    hp = R.hophip()
    members = STACKS[case]
    c = CASES[members[0][0]]
    want = [single(key)[idx] for key, idx in members]
    aus = [access_units(key)[idx] for key, idx in members]
    n = ((c["W"] + 63) // 64) * ((c["H"] + 63) // 64)
    ctx = hp.Context(c["W"], c["H"], bit_depth=c["bd"], pictures=len(members))     # no original is ever uploaded
    infos, match, parts, levels, sao = ctx.access_units_decode(aus)
    assert match == [[1, 1, 1]] * len(members), match
    for k, w in enumerate(want):
        assert bytes(infos[k]) == bytes(w["info"]), (case, k)
        assert parts[k * n:(k + 1) * n].tobytes() == w["parts"].tobytes(), (case, "parts", k)
        assert np.array_equal(levels[k * n:(k + 1) * n], w["levels"]), (case, "levels", k)
        assert (sao is None) == (w["sao"] is None) and (sao is None or sao[k * n:(k + 1) * n].tobytes() == w["sao"].tobytes()), (case, "sao", k)
    check_stack_against_singles(ctx, want, c["plain"], case)
    # the levels never asked for: the same pictures
    for comp in range(3):
        a = np.full((ctx.H >> (comp > 0), ctx.W >> (comp > 0)), 99, np.int16)
        ctx._chk(ctx.L.hop_recon_upload(ctx.h, comp, a.ctypes.data), "hop_recon_upload")
    infos2, match2, parts2, levels2, _ = ctx.access_units_decode(aus, want_levels=False)
    assert match2 == match and levels2 is None and parts2.tobytes() == parts.tobytes()
    check_stack_against_singles(ctx, want, c["plain"], case + ", levels NULL")
    assert ctx.access_units_decode(aus, want_outputs=False)[1] == match
    ctx.close()


def test_one_access_unit_on_an_unstacked_context():
    hp = R.hophip()
    want = single("64x64_sharp77")
    ctx = hp.Context(64, 64)
    infos, match, parts, levels, sao = ctx.access_units_decode(access_units("64x64_sharp77"))
    assert match == [[1, 1, 1]] and parts.tobytes() == want[0]["parts"].tobytes() and np.array_equal(levels, want[0]["levels"]) and sao.tobytes() == want[0]["sao"].tobytes()
    check_stack_against_singles(ctx, want, None, "unstacked")
    with pytest.raises(hp.HopError) as e:
        ctx.access_units_decode(access_units("64x64_sharp77") * 2)
    assert e.value.code == -1
    ctx.close()


@pytest.fixture(scope="module")
def coded_stack():
    """three different 192x128 pictures coded in a stack (wpp, lag 5, slots 16): parts, levels, the encoder's planes and SS reference before the loop filters, its final
    planes and the three access units"""
    hp = R.hophip()
    c = CASES["192x128_wpp_sao0"]
    pics = [lenslet(192, 128, 16, seed) for seed in (7, 21, 22)]
    st = hp.Context(192, 128, pictures=3, slots=16)
    st.upload_orig(st.stack([p[0] for p in pics]), st.stack([p[1] for p in pics], True), st.stack([p[2] for p in pics], True))
    parts = st.encode_frame(c["qp"], c["mi"], 0, None, wpp=1, wavefront_lag=5)[3]
    levels = st.levels_download()
    before, ss = planes(st), padded(st)
    st.deblock_frame(parts, c["qp"])
    final = planes(st)
    data, sizes = st.access_unit_write(parts, None, None, qp=c["qp"], slice_type=3, wpp=1, plain_intra=0, mi_size=c["mi"], hash=1)
    st.close()
    edges = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return dict(qp=c["qp"], parts=parts, levels=levels, before=before, ss=ss, final=final, aus=[data[edges[k]:edges[k + 1]] for k in range(3)])


def test_round_trip_on_the_device(coded_stack):
    """the three access units into a fresh stacked context that never saw an original: the encoder's final planes and levels; the parser takes the launches of ONE picture"""
    hp = R.hophip()
    dec = hp.Context(192, 128, pictures=3)
    dec.profile(on=True, reset=True)
    infos, match, parts, levels, sao = dec.access_units_decode(coded_stack["aus"])
    launches = dec.profile(read=hp.HOP_K_PARSE)[0]
    dec.profile(on=False)
    assert match == [[1, 1, 1]] * 3 and sao is None
    assert np.array_equal(levels, coded_stack["levels"])
    for comp in range(3):                                                    # (picture by picture: nobody writes the rows between them)
        for k, (a, b) in enumerate(zip(dec.unstack(dec.recon_download(comp), comp > 0), dec.unstack(coded_stack["final"][comp], comp > 0))):
            assert np.array_equal(a, b), ("picture", k, comp, np.argwhere(a != b)[:4])
    assert launches == 3 + 2 * (2 - 1), launches                             # wctu + 2 (hctu - 1), the same as one picture
    dec.close()


@pytest.mark.parametrize("schedule", (0, 1))
def test_decode_stack_alone(coded_stack, schedule):
    """hop_decode_stack on the encoder's parts and levels: its reconstruction before the loop filters and its whole padded SS planes"""
    hp = R.hophip()
    dec = hp.Context(192, 128, pictures=3)
    dec.decode_stack(coded_stack["parts"], coded_stack["levels"], qp=coded_stack["qp"], schedule=schedule)
    for comp in range(3):
        got = dec.recon_download(comp)
        for k, (a, b) in enumerate(zip(dec.unstack(got, comp > 0), dec.unstack(coded_stack["before"][comp], comp > 0))):
            assert np.array_equal(a, b), (schedule, "picture", k, comp, np.argwhere(a != b)[:4])
        s = dec.ssref_download(comp)
        assert np.array_equal(s, coded_stack["ss"][comp]), (schedule, "ssref", comp, np.argwhere(s != coded_stack["ss"][comp])[:4])
    # malformed partition data in picture 2: refused with the picture named, nothing enqueued
    before = padded(dec) + planes(dec)
    n = coded_stack["parts"].shape[0] // 3
    bad = coded_stack["parts"].copy()
    bad[2 * n]["luma_dir"][:] = 40; bad[2 * n]["pred_mode"][:] = 1; bad[2 * n]["part_size"][:] = 0
    with pytest.raises(hp.HopError) as e:
        dec.decode_stack(bad, coded_stack["levels"], qp=coded_stack["qp"], schedule=schedule)
    assert e.value.code == -1 and "picture 2" in str(e.value), e.value
    assert all(np.array_equal(a, b) for a, b in zip(before, padded(dec) + planes(dec)))
    dec.close()


def test_decode_stack_on_one_picture_is_decode_frame(coded_stack):
    hp = R.hophip()
    n = coded_stack["parts"].shape[0] // 3
    a, b = hp.Context(192, 128), hp.Context(192, 128)
    a.decode_stack(coded_stack["parts"][n:2 * n], coded_stack["levels"][n:2 * n], qp=coded_stack["qp"])
    b.decode_frame(coded_stack["parts"][n:2 * n], coded_stack["levels"][n:2 * n], qp=coded_stack["qp"])
    for x, y in zip(planes(a) + padded(a), planes(b) + padded(b)):
        assert np.array_equal(x, y)
    a.close(); b.close()


def test_refusals_leave_the_pictures_alone():
    hp = R.hophip()
    good = access_units("192x128_wpp")[0]
    ctx = hp.Context(192, 128, pictures=2)
    assert ctx.access_units_decode([good, good], want_outputs=False)[1] == [[1, 1, 1]] * 2
    before = padded(ctx) + planes(ctx)

    def refused(aus, *words, active=None):
        with pytest.raises(hp.HopError) as e:
            ctx.access_units_decode(aus, active, want_outputs=False)
        assert e.value.code == -1 and all(w in str(e.value) for w in words), (words, e.value)
        assert all(np.array_equal(a, b) for a, b in zip(before, padded(ctx) + planes(ctx))), words

    refused([good, access_units("192x128_seed7_mi15_wpp")[0]], "access unit 1", "mi_size")        # the micro-image sizes differ
    refused([good, access_units("192x128_wpp_sao0")[0]], "access unit 1", "SAO")                # the SAO flags differ (the SPS's, then the slice's)
    refused([good], "1 access unit")
    refused([good, good, good], "3 access units")
    assert ctx.access_units_decode([good, good], want_outputs=False)[1] == [[1, 1, 1]] * 2
    ctx.close()
    # an access unit without parameter sets that neither an earlier one nor `active` supplies: refused; with `active` it is read
    later = access_units("128x64_2frames")[1]
    want = single("128x64_2frames")
    ctx = hp.Context(128, 64, pictures=2)
    with pytest.raises(hp.HopError) as e:
        ctx.access_units_decode([later, later])
    assert e.value.code == -1 and "access unit 0" in str(e.value) and "parameter sets" in str(e.value), e.value
    infos, match = ctx.access_units_decode([later, later], want[0]["info"], want_outputs=False)[:2]
    assert match == [[1, 1, 1]] * 2 and [i.params.parameter_sets for i in infos] == [0, 0] and [i.params.poc for i in infos] == [1, 1]
    check_stack_against_singles(ctx, [want[1], want[1]], None, "active from the caller")
    ctx.close()


def test_one_flipped_slice_data_byte_in_access_unit_1():
    """either an error that names access unit 1, or a hash mismatch of picture 1 alone; the context decodes on"""
    hp = R.hophip()
    au = access_units("192x128_wpp")[0]
    ctx = hp.Context(192, 128, pictures=2)
    info = ctx.access_units_decode([au, au], want_outputs=False)[0][0]
    vcl_at = [p + len(u) - len(u.lstrip(b"\x00")) + 1 for p, u, t in S.split_units(au) if t < 32][0]
    for off in (40, 500):
        at = vcl_at + info.header_bytes + off
        bad = au[:at] + bytes([au[at] ^ 0x55]) + au[at + 1:]
        try:
            match = ctx.access_units_decode([au, bad], want_outputs=False)[1]
            assert match[0] == [1, 1, 1] and match[1] != [1, 1, 1], (off, match)
        except hp.HopError as e:
            assert e.code == -1 and "access unit 1" in str(e), e
        assert ctx.access_units_decode([au, au], want_outputs=False)[1] == [[1, 1, 1]] * 2
    ctx.close()
