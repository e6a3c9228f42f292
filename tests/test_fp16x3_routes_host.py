"""The fp16x3 GEMM routing decides today what it decided before its last change: for every case of
tests/fp16x3_route_cases.py the built library's f2g_gemm_f16_ok and f2g_gemm_colsum_part_rows and the route ops.gemm's
chooser picks (ops._fp16x3_route: no image is built, nothing is launched) equal tests/golden/fp16x3_route_answers.json,
which was recorded from the parent commit by `fp16x3_route_cases.py --record` against a checkout and build of it."""
import ctypes as C
import json

import pytest

import fp16x3_route_cases as cases


@pytest.fixture(scope="module")
def golden():
    with open(cases.GOLDEN) as f:
        return json.load(f)["answers"]


def test_the_table_is_not_empty(golden):
    """every kernel is accepted as fp32 (2, where it has images to make) and as handed over (1) and declines at least
    ten distinct cases; the partial-row answers have both tile heights and 0; the case list is the generator's"""
    assert list(golden) == cases.case_ids() and len(set(golden)) == len(golden) >= 1000
    for name, (_, _, _, _, images) in cases.BASES.items():
        ok = [row[0] for cid, row in golden.items() if cid.startswith(name + ": ")]
        assert 1 in ok and ok.count(0) >= 10, name
        assert (2 in ok) == any(images), name
        assert golden[f"{name}: base"][3 if name == "PLAIN" else 2] == name, name      # the chooser reaches every route
    with cases.host_setup(ops()):
        M = {name: cases.build(ops(), name, {}, [], True)[0].A.rows for name in cases.BASES}
    parts = {name: golden[f"{name}: base"][1] for name in cases.BASES}
    assert parts["TAP"] == 4 * -(-M["TAP"] // 256) and parts["TAP3"] == 4 * -(-M["TAP3"] // 256)
    assert parts["TAP3N"] == 2 * -(-M["TAP3N"] // 128) and parts["TAPN"] == 0 and parts["PLAIN"] == 0
    assert 0 in {row[1] for cid, row in golden.items() if cid.startswith("TAP: ")}


def ops():
    from flow2gan_amd import ops
    return ops


def test_the_decisions_equal_the_recorded_ones(golden):
    from flow2gan_amd import _lib
    got = cases.answers(ops(), _lib)
    wrong = {cid: (got.get(cid), want) for cid, want in golden.items() if got.get(cid) != want}
    assert not wrong and len(got) == len(golden), dict(list(wrong.items())[:20])


def test_the_chooser_builds_no_image():
    """ops._fp16x3_route leaves the descriptor marked for the kernel and stops there: an image builder or a launch
    under it raises (cases.host_setup)"""
    o = ops()
    with cases.host_setup(o):
        def boom(operand):
            raise AssertionError("an image builder ran")
        o._FP16X3_ROUTES = {key: tuple(r._replace(images=tuple(f and boom for f in r.images)) for r in rs)
                            for key, rs in o._FP16X3_ROUTES.items()}
        for k in cases.thresholds(o):
            setattr(o, k, 1)
        d, A, Bm, out = cases.build(o, "TAP3N", cases.CHIP_FILLING["TAP3N"], [], False)
        r = o._fp16x3_route(d, A, Bm, out, 0, False, 1, 0, False, None)
        assert r.counter == "FP16X3_TAP3N_LAUNCHES" and (d.A.split, d.B.split, d.precision) == (8, 0, 4)
        assert (A.split, Bm.split) == (0, 0) and C.addressof(d.A) != C.addressof(A)
        with pytest.raises(AssertionError, match="an image builder ran"):
            o._fp16x3_gemm(d, A, Bm, out, 0, False, 1, 0, False, None)


def test_the_first_image_lives_until_the_second_is_built():
    """an image belongs to the temporary operand its builder returns (d.A = ... copies the fields only): if that one
    were dropped before the other image is allocated, the allocator could hand the same memory out twice"""
    import weakref
    o = ops()

    class Image:
        pass
    with cases.host_setup(o):
        built = []

        def image(operand):
            assert all(ref() is not None for ref in built), "the first image was dropped before the second was built"
            n, buf = o.Operand(), Image()
            C.memmove(C.byref(n), C.byref(operand), C.sizeof(o.Operand))
            n._keep = (buf,)
            built.append(weakref.ref(buf))
            return n
        o._FP16X3_ROUTES = {key: tuple(r._replace(images=tuple(f and image for f in r.images)) for r in rs)
                            for key, rs in o._FP16X3_ROUTES.items()}
        o.FP16X3_MIN_K = o.FP16X3_MIN_N = 1
        d, A, Bm, out = cases.build(o, "PLAIN", {}, [], False)
        n0 = o.FP16X3_LAUNCHES
        assert o._fp16x3_gemm(d, A, Bm, out, 0, False, 1, 0, False, None)
        assert len(built) == 2 and o.FP16X3_LAUNCHES == n0 + 1
