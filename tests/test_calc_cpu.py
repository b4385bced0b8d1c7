"""CPU tests of the band math: the parser and its refusals, the numpy rule (``calc.calc_arrays``) against a brute-force
per-pixel loop over Python floats, the two validators (``calc.validate`` and the library's ``fra_calc_check``) against
each other on random almost-valid programs, and the ABI.  No GPU: ``fra_calc_check`` is pure host code."""
import math
import re
import struct
from pathlib import Path

import numpy as np
import pytest

from flac_raster import _native as N
from flac_raster import calc
from flac_raster.calc import Program, calc_arrays, compile_exprs

ROOT = Path(__file__).resolve().parents[1]
DTYPES = [np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64]


# ------------------------------------------------------------------------------- the brute force
def _f(x):
    return float(x)


def _run_pixel(prog, px, nodata, fill):
    """The program on one pixel (a list of Python floats, one per band): Python-float arithmetic, IEEE by hand where
    Python raises.  Returns the f64 result per output and whether the pixel is left out."""
    def div(a, b):
        if b == 0.0:
            if a != a or a == 0.0:
                return math.nan
            return math.copysign(math.inf, a) * math.copysign(1.0, b)
        try:
            return a / b
        except OverflowError:
            return math.copysign(math.inf, a) * math.copysign(1.0, b)

    def mul(a, b):
        try:
            return a * b
        except OverflowError:
            return math.copysign(math.inf, a) * math.copysign(1.0, b)

    def add(a, b):
        try:
            return a + b
        except OverflowError:
            return math.copysign(math.inf, a if abs(a) > abs(b) else b)

    left = False
    if nodata is not None:
        for b in prog.bands_read():
            left |= px[b] != px[b] or px[b] == nodata
    out = {}
    st = []
    for op, arg in prog.words():
        if op == calc.CONST:
            st.append(float(prog.consts[arg]))
        elif op == calc.BAND:
            st.append(px[arg])
        elif op == calc.STORE:
            v = st.pop()
            out[arg] = fill if left else v
        elif op == calc.NEG:
            st.append(-st.pop())
        elif op == calc.ABS:
            st.append(abs(st.pop()))
        elif op == calc.SQRT:
            x = st.pop()
            st.append(math.nan if x != x or x < 0.0 else (x if x in (0.0, math.inf) else math.sqrt(x)))
        elif op == calc.FLOOR:
            x = st.pop()
            st.append(x if x != x or math.isinf(x) or x == 0.0 else math.copysign(float(math.floor(x)), x)
                      if math.floor(x) == 0 else float(math.floor(x)))
        elif op == calc.NOT:
            st.append(0.0 if st.pop() != 0.0 else 1.0)
        elif op == calc.SELECT:
            b, a, c = st.pop(), st.pop(), st.pop()
            st.append(a if c != 0.0 else b)
        else:
            b, a = st.pop(), st.pop()
            r = {calc.ADD: lambda: add(a, b), calc.SUB: lambda: add(a, -b), calc.MUL: lambda: mul(a, b),
                 calc.DIV: lambda: div(a, b), calc.MIN: lambda: a if a < b else b, calc.MAX: lambda: a if a > b else b,
                 calc.LT: lambda: _f(a < b), calc.LE: lambda: _f(a <= b), calc.GT: lambda: _f(a > b),
                 calc.GE: lambda: _f(a >= b), calc.EQ: lambda: _f(a == b), calc.NE: lambda: _f(a != b),
                 calc.AND: lambda: _f(a != 0.0 and b != 0.0), calc.OR: lambda: _f(a != 0.0 or b != 0.0)}[op]()
            st.append(r)
    assert not st
    return out, left


def _convert_scalar(v, dt):
    """One f64 result in ``dt`` by the rule, as the element's bytes."""
    dt = np.dtype(dt)
    if dt.kind == "f":
        if v != v:
            return struct.pack("<d", math.nan) if dt.itemsize == 8 else struct.pack("<f", math.nan)
        if dt.itemsize == 8:
            return struct.pack("<d", v)
        try:
            return struct.pack("<f", v)
        except OverflowError:
            return struct.pack("<f", math.copysign(math.inf, v))
    info = np.iinfo(dt)
    if v != v:
        r = 0
    elif math.isinf(v):
        r = info.max if v > 0 else info.min
    else:
        r = min(max(round(v), info.min), info.max)  # Python's round: half to even
    return np.array(r, dt).tobytes()


def _brute(a, prog, odt, nodata=None, fill=math.nan):
    nb, h, w = a.shape
    out = np.zeros((prog.nout, h, w), odt)
    flat = out.view(np.uint8).reshape(prog.nout, h, w, np.dtype(odt).itemsize)
    n = 0
    for r in range(h):
        for c in range(w):
            res, left = _run_pixel(prog, [float(a[b, r, c]) for b in range(nb)], nodata, fill)
            n += left
            for k, v in res.items():
                flat[k, r, c] = np.frombuffer(_convert_scalar(v, odt), np.uint8)
    return out, n


def _raster(dt, rng, shape=(4, 7, 19)):
    dt = np.dtype(dt)
    small = rng.integers(0, 4, size=shape)
    if dt.kind != "f":
        info = np.iinfo(dt)
        full = rng.integers(info.min, int(info.max) + 1, size=shape, dtype=np.int64)
        return np.where(rng.random(shape) < 0.5, small, full).astype(dt)
    full = rng.normal(0.0, 1.0, size=shape) * 10.0 ** rng.integers(-3, 6, size=shape)
    a = np.where(rng.random(shape) < 0.5, small.astype(np.float64), full).astype(dt)
    flat = a.reshape(-1)
    k = rng.choice(flat.size, size=24, replace=False)
    flat[k] = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0], dt), k.size)
    return a


def _same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got.view(np.uint8) != want.view(np.uint8))[:3])


# ------------------------------------------------------------------------------- the parser
def _eval1(expr, bands, odt=np.float64):
    """The compiled expression on one pixel."""
    a = np.array(bands, np.float64).reshape(len(bands), 1, 1)
    return float(calc_arrays(a, compile_exprs([expr], len(bands)), odt)[0][0, 0, 0])


@pytest.mark.parametrize("expr", [
    "b1 - b2 - b3", "b1 / b2 / b3", "b1 - b2 * b3 + b4", "b1 * (b2 + b3) / b4", "-b1 * b2", "-(b1 - b2) - -b3",
    "b1 + b2 * -b3 / b4 - 2.5", "(b1 - b2) / (b1 + b2)", "b1 - (b2 - (b3 - b4))", "1e3 * b1 - 7 + 0.125 * b4",
    "b1 < b2", "b1 + 1 >= b2 * 2", "b1 == b2 - 2", "b1 != b1", "not b1 > b2", "b1 < b2 and b3 < b4 or b1 == 7",
    "b1 > b2 or b3 < b4 and b2 > b3", "not (b1 < b2 or b3 > b4)", "abs(b1 - b2 * b3)", "min(b1, b2) - max(b3, b4)",
])
def test_precedence_and_associativity_follow_python(expr):
    for bands in ([7.0, 3.0, 2.0, 5.0], [1.5, -4.0, 8.0, 0.5], [3.0, 3.0, 3.0, 3.0]):
        env = dict(zip(("b1", "b2", "b3", "b4"), bands), abs=abs, min=min, max=max)
        want = float(eval(expr, {"__builtins__": {}}, env))  # True / False become 1.0 / 0.0, as the rule says
        assert _eval1(expr, bands) == want, (expr, bands)


def test_every_whitelisted_form():
    b = [9.0, 2.0, -3.5, 0.0]
    assert _eval1("sqrt(b1)", b) == 3.0 and _eval1("floor(b3)", b) == -4.0 and _eval1("abs(b3)", b) == 3.5
    assert _eval1("min(b1, b2)", b) == 2.0 and _eval1("max(b1, b2)", b) == 9.0
    assert _eval1("where(b4, b1, b2)", b) == 2.0 and _eval1("where(b3, b1, b2)", b) == 9.0
    assert _eval1("clamp(b1, 0, 5)", b) == 5.0 and _eval1("clamp(b3, 0, 5)", b) == 0.0 and _eval1("clamp(b2, 0, 5)", b) == 2.0
    assert _eval1("b1 and b2", b) == 1.0 and _eval1("b1 and b4", b) == 0.0 and _eval1("b4 or b3", b) == 1.0
    assert _eval1("not b4", b) == 1.0 and _eval1("not b3", b) == 0.0
    assert _eval1("b1 and b2 and b4", b) == 0.0 and _eval1("b4 or b4 or b2", b) == 1.0
    assert math.isnan(_eval1("b4 / b4", b)) and _eval1("b1 / b4", b) == math.inf and _eval1("-b1 / b4", b) == -math.inf
    assert _eval1("3", b) == 3.0 and _eval1("-2.5e0", b) == -2.5 and _eval1("  b2  ", b) == 2.0
    # the spec is the < / > form, not minNum; NaN is true
    assert math.isnan(_eval1("min(1, b4 / b4)", b)) and _eval1("min(b4 / b4, 1)", b) == 1.0
    assert math.isnan(_eval1("max(1, b4 / b4)", b)) and _eval1("max(b4 / b4, 1)", b) == 1.0
    assert _eval1("where(b4 / b4, 1, 2)", b) == 1.0 and _eval1("not b4 / b4", b) == 0.0
    # nothing is folded: what is written is what is evaluated
    p = compile_exprs(["1 + 2 * 3"], 1)
    assert [o for o, _ in p.words()] == [calc.CONST, calc.CONST, calc.CONST, calc.MUL, calc.ADD, calc.STORE]
    assert p.consts.tolist() == [1.0, 2.0, 3.0]
    p = compile_exprs(["b1", "b2 - b1", "b1 * 2"], 2)  # one program, one STORE per expression
    assert [(o, a) for o, a in p.words() if o == calc.STORE] == [(calc.STORE, 0), (calc.STORE, 1), (calc.STORE, 2)]
    assert p.nout == 3 and p.bands_read() == [0, 1]
    assert str(compile_exprs(["clamp(b1, 0, 1)"], 1)) == "BAND 0 CONST 0 MAX CONST 1 MIN STORE 0"


@pytest.mark.parametrize("expr,what", [
    ("x + 1", "x"), ("b0", "b0"), ("b5", "b5"), ("b01", "b01"), ("B1", "B1"), ("b1.real", "b1.real"), ("b1[0]", "b1[0]"),
    ("lambda: b1", "lambda"), ("'a'", "'a'"), ("b1 < b2 < b3", "b1 < b2 < b3"), ("b1 ** 2", "b1 ** 2"),
    ("b1 % 2", "b1 % 2"), ("b1 // 2", "b1 // 2"), ("exp(b1)", "exp(b1)"), ("__import__('os')", "__import__"),
    ("b1 if b2 else b3", "b1 if b2 else b3"), ("abs(b1, b2)", "abs(b1, b2)"), ("min(b1)", "min(b1)"),
    ("where(b1, b2)", "where(b1, b2)"), ("clamp(b1, 0)", "clamp(b1, 0)"), ("max(b1, b2, b3)", "max(b1, b2, b3)"),
    ("True", "True"), ("1j", "1j"), ("~b1", "~b1"), ("+b1", "+b1"), ("b1 is b2", "b1 is b2"), ("b1 in b2", "b1 in b2"),
    ("abs(x=b1)", "abs(x=b1)"), ("(b1).__class__", "__class__"), ("b1 +", "b1 +"), ("", "''"), ("b1; b2", "b1; b2"),
    ("[b1]", "[b1]"), ("(b1, b2)", "(b1, b2)"), ("b1 := 2", "b1 := 2"), ("abs.__call__(b1)", "abs.__call__"),
])
def test_refusals_name_the_offending_text(expr, what):
    with pytest.raises(ValueError, match=re.escape(what)):
        compile_exprs([expr], 4)


def test_limits_are_refused():
    deep = "b1 + (b1 + (b1 + (b1 + (b1 + (b1 + (b1 + (b1 + b1)))))))"  # nine operands before the first ADD
    with pytest.raises(ValueError, match="stack deeper than 8"):
        compile_exprs([deep], 1)
    assert calc.validate(compile_exprs(["b1 + (b1 + (b1 + (b1 + (b1 + (b1 + (b1 + b1))))))"], 1), 1) == 8
    assert compile_exprs([" + ".join(["b1"] * 64)], 1).code.size == 128
    with pytest.raises(ValueError, match="more than 128 words"):
        compile_exprs([" + ".join(["b1"] * 65)], 1)
    with pytest.raises(ValueError, match="more than 128 words"):
        compile_exprs([" + ".join(["b1"] * 40)] * 2, 1)
    assert compile_exprs([" + ".join(str(k) for k in range(32))], 1).consts.size == 32
    assert compile_exprs([" + ".join(str(k % 32) for k in range(50))], 1).consts.size == 32  # equal constants share
    with pytest.raises(ValueError, match="more than 32 constants"):
        compile_exprs([" + ".join(str(k) for k in range(33))], 1)
    assert compile_exprs(["b1"] * 8, 1).nout == 8
    with pytest.raises(ValueError, match="9 expressions"):
        compile_exprs(["b1"] * 9, 1)
    with pytest.raises(ValueError, match="0 expressions"):
        compile_exprs([], 1)
    with pytest.raises(ValueError):
        compile_exprs(["b1"], 0)
    with pytest.raises(ValueError):
        compile_exprs(["b1"], 256)
    p = compile_exprs(["0.0 + -0.0"], 1)  # 0.0 and -0.0 are two constants; the minus is an op on a third
    assert p.consts.size == 1 and [o for o, _ in p.words()] == [calc.CONST, calc.CONST, calc.NEG, calc.ADD, calc.STORE]


# ------------------------------------------------------------------------------- the reference
def _all_ops_program():
    """Every op at least once, two outputs."""
    e1 = "where(b1 > b2 and not b3 == 0 or b4 <= 1, floor(sqrt(abs(b1))) * 0.5, -min(b2, max(b3, 0.5)) / b4)"
    e2 = "(b1 < b2) + (b2 >= b3) - (b3 != b4) + clamp(b4 - b1, -10, 1e30)"
    p = compile_exprs([e1, e2], 4)
    assert {o for o, _ in p.words()} == set(range(len(calc.OPS)))
    return p


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: np.dtype(d).name)
def test_calc_arrays_equals_the_per_pixel_loop(dt):
    rng = np.random.default_rng(100 + np.dtype(dt).num)
    a = _raster(dt, rng)
    prog = _all_ops_program()
    ndvi = compile_exprs(["(b4 - b3) / (b4 + b3)", "b2 * 1e30"], 4)
    nd = 3.0
    for odt in DTYPES:
        for p in (prog, ndvi):
            got, left = calc_arrays(a, p, odt)
            want, n = _brute(a, p, odt)
            _same(got, want, (np.dtype(dt), np.dtype(odt)))
            assert left.tolist() == [0, 0] and n == 0
        for nodata, fill in ((nd, calc.default_fill(odt)), (nd, 300.5), (math.nan, -1.0), (123456.0, 1.0)):
            got, left = calc_arrays(a, ndvi, odt, nodata, fill)
            want, n = _brute(a, ndvi, odt, nodata, fill)
            _same(got, want, (np.dtype(dt), np.dtype(odt), nodata, fill))
            assert left.tolist() == [n, n]
    # the nodata rule looks at the bands the program reads, and at no other
    only2 = compile_exprs(["b2 + 0"], 4)
    x2 = a[1].astype(np.float64)
    assert calc_arrays(a, only2, np.float32, nd)[1].tolist() == [int(np.count_nonzero((x2 == nd) | np.isnan(x2)))]
    assert calc_arrays(a, ndvi, np.float32, nd)[1][0] >= calc_arrays(a, only2, np.float32, nd)[1][0]


def test_output_conversion():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 254.5, 255.5, 1e30, -1e30, np.inf, -np.inf, np.nan, -0.0, 3.4e38, 3.5e38])
    assert calc.convert(v, np.uint8).tolist() == [0, 2, 2, 0, 0, 254, 255, 255, 0, 255, 0, 0, 0, 255, 255]
    assert calc.convert(v, np.int8).tolist() == [0, 2, 2, 0, -2, 127, 127, 127, -128, 127, -128, 0, 0, 127, 127]
    assert calc.convert(v, np.int32)[7:12].tolist() == [2**31 - 1, -2**31, 2**31 - 1, -2**31, 0]
    assert calc.convert(v, np.uint32)[7:12].tolist() == [2**32 - 1, 0, 2**32 - 1, 0, 0]
    f = calc.convert(v, np.float32)
    assert f[7] == np.float32(1e30) and f[9] == np.inf and f[10] == -np.inf and f[13] == np.float32(3.4e38) and f[14] == np.inf
    assert f.view(np.uint32)[11] == 0x7FC00000 and f.view(np.uint32)[12] == 0x80000000
    neg_nan = np.array([-np.nan, np.nan]).view(np.uint64) | np.uint64(1 << 63 | 5)  # any sign, any payload
    assert calc.convert(neg_nan.view(np.float64), np.float64).view(np.uint64).tolist() == [0x7FF8000000000000] * 2
    assert calc.default_fill(np.float32) != calc.default_fill(np.float32) and calc.default_fill(np.int16) == 0.0


# ------------------------------------------------------------------------------- the validators
def _valid_programs(rng):
    exprs = ["(b4 - b3) / (b4 + b3)", "where(b1 > 2 and not b2, clamp(b1 * 0.5, 1, 200), -sqrt(abs(b2)))", "b1", "7",
             "b1 - (b2 * (b3 + (b4 / (b1 - (b2 * (b3 + b4))))))", "floor(b1 / 3) != b2 or b3 <= b4", " + ".join(["b2"] * 64),
             "min(b1, max(b2, 1.5)) == 2"]
    progs = [compile_exprs([e], 4) for e in exprs]
    progs.append(compile_exprs(exprs[:4], 4))
    progs.append(compile_exprs(["b1"] * 8, 4))
    return progs


def _native_ok(prog, nbands, flags=None):
    p = N.calc_program(prog)
    if flags is not None:
        p.flags = flags
    rc = N.load().fra_calc_check(p, nbands)
    assert rc in (0, -1)
    msg = N.load().fra_last_error().decode() if rc else ""
    return rc == 0, msg


def test_validators_agree_on_random_almost_valid_programs():
    rng = np.random.default_rng(77)
    base = _valid_programs(rng)
    nops = len(calc.OPS)
    seen = {True: 0, False: 0}
    for n in range(4000):
        src = base[int(rng.integers(len(base)))]
        code = src.code.copy()
        consts, nout, nbands = src.consts.copy(), src.nout, 4
        for _ in range(int(rng.integers(0, 4))):  # a few mutations of a valid program
            kind = int(rng.integers(9))
            i = int(rng.integers(code.size)) if code.size else 0
            if kind == 0 and code.size:
                code[i] = rng.integers(0, nops + 2) | (int(rng.integers(0, 6)) << 8 if rng.random() < 0.7 else 0)
            elif kind == 1 and code.size:
                code = np.delete(code, i)
            elif kind == 2 and code.size < 140:
                code = np.insert(code, i, rng.integers(0, nops) | (int(rng.integers(0, 3)) << 8 if rng.random() < 0.5 else 0))
            elif kind == 3 and code.size > 1:
                j = int(rng.integers(code.size))
                code[i], code[j] = code[j], code[i]
            elif kind == 4:
                nout = int(rng.integers(0, 10))
            elif kind == 5:
                consts = consts[: int(rng.integers(0, consts.size + 1))]
            elif kind == 6:
                nbands = int(rng.choice([0, 1, 2, 3, 4, 5, 255, 256]))
            elif kind == 7 and code.size:
                code[i] = (code[i] & 0xFF) | int(rng.integers(0, 256)) << 8
            elif kind == 8 and code.size:
                code = np.concatenate([code, code[: int(rng.integers(1, code.size + 1))]])
        if code.size > 128 or consts.size > 32:
            # the wire format cannot carry it: both sides refuse by the count
            with pytest.raises(ValueError, match="outside"):
                calc.validate(Program(code, consts, nout), nbands)
            continue
        prog = Program(code, consts, nout)
        try:
            calc.validate(prog, nbands)
            ok, why = True, ""
        except ValueError as e:
            ok, why = False, str(e)
        nat, msg = _native_ok(prog, nbands)
        assert nat == ok and msg == why, (str(prog), nout, nbands, why, msg)
        seen[ok] += 1
        if ok:  # a valid program runs
            a = rng.integers(0, 50, size=(nbands, 2, 3)).astype(np.int16)
            out, left = calc_arrays(a, prog, np.float32, nodata=7.0)
            assert out.shape == (nout, 2, 3) and left.shape == (nout,)
    assert seen[True] > 500 and seen[False] > 1500, seen
    ndvi = base[0]
    assert _native_ok(ndvi, 4, flags=1)[0] and _native_ok(ndvi, 4, flags=0)[0]
    ok, msg = _native_ok(ndvi, 4, flags=2)
    assert not ok and "flags" in msg
    for v in (math.nan, math.inf, -math.inf):  # any double is a constant, a nodata value, a fill
        p = N.calc_program(Program([calc.CONST, calc.STORE], [v], 1), nodata=v, fill=v)
        assert N.load().fra_calc_check(p, 1) == 0
    assert N.load().fra_calc_check(None, 4) == -1


# ------------------------------------------------------------------------------- the ABI
def test_abi_names_and_layout():
    header = (ROOT / "include" / "flac_raster_amd.h").read_text()
    for name in ("fra_calc_check", "fra_calc", "fra_decode_device_calc", "fra_calc_timing"):
        assert name in N.EXPORTS and re.search(rf"FRA_API int {name}\(", header), name
        assert hasattr(N.load(), name)
    for name in ("fra_calc_program", "fra_calc_dst", "fra_calc_job", "FRA_CALC_NODATA"):
        assert name in header
    assert N.load().fra_abi_version() == 3
    import ctypes as C

    assert C.sizeof(N.CalcProgram) == 544 and N.CalcProgram.code.offset == 32 and N.CalcProgram.consts.offset == 288
    assert C.sizeof(N.CalcDst) == 40 and C.sizeof(N.CalcJob) == 56 + 544 + 40 and N.CalcJob.program.offset == 56
    for k, name in enumerate(calc.OPS):  # the op numbers of the header are those of calc.py
        assert re.search(rf"FRA_CALC_{name} = {k}\b", header), name
    assert (calc.MAX_CODE, calc.MAX_CONST, calc.MAX_OUT, calc.MAX_DEPTH) == (128, 32, 8, 8)
    ms = C.c_float(-1.0)
    assert N.load().fra_calc_timing(C.byref(ms)) == 0 and ms.value >= 0.0
    assert N.load().fra_calc_timing(None) == -1
