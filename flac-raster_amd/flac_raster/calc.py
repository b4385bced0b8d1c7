"""Band math: per-pixel expressions over the bands of a raster.

The rule of ``fra_calc`` / ``fra_decode_device_calc`` (the normative text is in ``include/flac_raster_amd.h``), in numpy:
the GPU is checked against :func:`calc_arrays` bit for bit, never against itself.

An expression is Python syntax over the names ``b1 ... bN`` (1-based, as in ``gdal_calc`` and rasterio), numeric
constants, ``+ - * /`` (true division), unary ``-``, one comparison ``< <= > >= == !=``, ``and / or / not`` and the calls
``abs(x) sqrt(x) floor(x) min(a, b) max(a, b) where(c, a, b) clamp(x, lo, hi)``.  :func:`compile_exprs` lowers one
expression per output band into one stack program in reverse Polish notation -- nothing is folded: what is written is
what is evaluated -- and the program is the wire format: ``code[i] = op | arg << 8``.

Semantics.  Every element is taken as f64 and every op is one IEEE f64 operation.  Comparisons and the logic ops give
1.0 / 0.0; a value is true when ``x != 0.0`` (so NaN is true); ``MIN(a, b) = a < b ? a : b``, ``MAX(a, b) = a > b ? a :
b`` (not minNum), ``SELECT(c, a, b) = c != 0 ? a : b``.  A result goes to a float dtype by a plain cast, a NaN as the
quiet NaN ``0x7ff8000000000000``; to an integer dtype by round-half-even, then saturation, NaN -> 0.  With a nodata
value a pixel is left out when any band *the program reads* holds it (``float(x) == nodata``) or NaN; every output band
of such a pixel gets ``fill``, converted by the same rule; a NaN nodata matches nothing.
"""
from __future__ import annotations

import ast
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

MAX_CODE, MAX_CONST, MAX_OUT, MAX_DEPTH = 128, 32, 8, 8
FLAG_NODATA = 1

OPS = ("CONST", "BAND", "STORE", "ADD", "SUB", "MUL", "DIV", "NEG", "ABS", "SQRT", "FLOOR", "MIN", "MAX", "LT", "LE",
       "GT", "GE", "EQ", "NE", "AND", "OR", "NOT", "SELECT")
(CONST, BAND, STORE, ADD, SUB, MUL, DIV, NEG, ABS, SQRT, FLOOR, MIN, MAX, LT, LE, GT, GE, EQ, NE, AND, OR, NOT,
 SELECT) = range(len(OPS))
_UNARY = (NEG, ABS, SQRT, FLOOR, NOT)

DTYPES = ("uint8", "int8", "uint16", "int16", "uint32", "int32", "float32", "float64")


def pops_of(op: int) -> int:
    """Values a word pops (-1: an unknown op); every op but ``STORE`` pushes one."""
    if op in (CONST, BAND):
        return 0
    if op == STORE or op in _UNARY:
        return 1
    if op == SELECT:
        return 3
    return 2 if ADD <= op <= OR else -1


@dataclass
class Program:
    """A band-math program: ``code`` (uint16 words, ``op | arg << 8``), ``consts`` (f64) and ``nout`` outputs."""

    code: np.ndarray
    consts: np.ndarray
    nout: int

    def __post_init__(self):
        self.code = np.asarray(self.code, dtype=np.uint16).reshape(-1)
        self.consts = np.asarray(self.consts, dtype=np.float64).reshape(-1)
        self.nout = int(self.nout)

    def words(self) -> List[Tuple[int, int]]:
        return [(int(w) & 0xFF, int(w) >> 8) for w in self.code]

    def bands_read(self) -> List[int]:
        """The 0-based bands the program reads, ascending."""
        return sorted({a for o, a in self.words() if o == BAND})

    def __str__(self):
        return " ".join(OPS[o] + (f" {a}" if o in (CONST, BAND, STORE) else "") if o < len(OPS) else f"?{o}"
                        for o, a in self.words())


def validate(program: Program, nbands: int) -> int:
    """The Python twin of the C validator (``fra_calc_check``): ``ValueError`` naming the word for whatever it refuses;
    returns the deepest the stack gets."""
    ncode, nconst, nout = program.code.size, program.consts.size, program.nout
    if not 1 <= ncode <= MAX_CODE:
        raise ValueError(f"program of {ncode} words outside 1 ... {MAX_CODE}")
    if not 0 <= nconst <= MAX_CONST:
        raise ValueError(f"{nconst} constants outside 0 ... {MAX_CONST}")
    if not 1 <= nout <= MAX_OUT:
        raise ValueError(f"{nout} outputs outside 1 ... {MAX_OUT}")
    if not 1 <= nbands <= 255:
        raise ValueError(f"{nbands} source bands outside 1 ... 255")
    depth = deepest = 0
    stored = set()
    for i, (op, arg) in enumerate(program.words()):
        pops = pops_of(op)
        if pops < 0:
            raise ValueError(f"word {i}: unknown op {op}")
        if op == BAND:
            if arg >= nbands:
                raise ValueError(f"word {i}: band {arg} of {nbands}")
        elif op == CONST:
            if arg >= nconst:
                raise ValueError(f"word {i}: constant {arg} of {nconst}")
        elif op == STORE:
            if arg >= nout:
                raise ValueError(f"word {i}: output {arg} of {nout}")
            if arg in stored:
                raise ValueError(f"word {i}: output {arg} stored twice")
            stored.add(arg)
        elif arg:
            raise ValueError(f"word {i}: op {op} takes no argument ({arg})")
        if depth < pops:
            raise ValueError(f"word {i}: stack underflow")
        depth += (0 if op == STORE else 1) - pops
        if depth > MAX_DEPTH:
            raise ValueError(f"word {i}: stack deeper than {MAX_DEPTH}")
        deepest = max(deepest, depth)
    if depth:
        raise ValueError(f"word {ncode - 1}: {depth} values left on the stack at the end")
    for k in range(nout):
        if k not in stored:
            raise ValueError(f"word {ncode - 1}: output {k} is never stored")
    return deepest


_BINOPS = {ast.Add: ADD, ast.Sub: SUB, ast.Mult: MUL, ast.Div: DIV}
_CMPOPS = {ast.Lt: LT, ast.LtE: LE, ast.Gt: GT, ast.GtE: GE, ast.Eq: EQ, ast.NotEq: NE}
_CALLS = {"abs": (1, (ABS,)), "sqrt": (1, (SQRT,)), "floor": (1, (FLOOR,)), "min": (2, (MIN,)), "max": (2, (MAX,)),
          "where": (3, (SELECT,))}


class _Lowering:
    def __init__(self, nbands: int):
        self.nbands = nbands
        self.code: List[int] = []
        self.consts: List[float] = []

    def emit(self, op: int, arg: int = 0):
        self.code.append(op | arg << 8)

    def bad(self, expr: str, node, why: str):
        seg = ast.get_source_segment(expr, node) if hasattr(node, "lineno") else None
        raise ValueError(f"{why}: {seg or type(node).__name__!r} in {expr!r}")

    def const(self, v) -> int:
        # one entry per distinct bit pattern (0.0 and -0.0 differ, every NaN is kept as written)
        bits = np.float64(v).view(np.uint64)
        for k, c in enumerate(self.consts):
            if np.float64(c).view(np.uint64) == bits:
                return k
        self.consts.append(float(v))
        if len(self.consts) > MAX_CONST:
            raise ValueError(f"more than {MAX_CONST} constants")
        return len(self.consts) - 1

    def lower(self, expr: str, n):
        if isinstance(n, ast.Constant):
            if isinstance(n.value, bool) or not isinstance(n.value, (int, float)):
                self.bad(expr, n, "only numeric constants are allowed")
            self.emit(CONST, self.const(float(n.value)))
        elif isinstance(n, ast.Name):
            name = n.id
            if not (name[:1] == "b" and name[1:].isdigit() and name[1:2] != "0" and name[1:].isascii()):
                self.bad(expr, n, f"unknown name (the bands are b1 ... b{self.nbands})")
            b = int(name[1:])
            if b > self.nbands:
                self.bad(expr, n, f"band {b} of {self.nbands}")
            self.emit(BAND, b - 1)
        elif isinstance(n, ast.BinOp):
            if type(n.op) not in _BINOPS:
                self.bad(expr, n, "unsupported operator")
            self.lower(expr, n.left)
            self.lower(expr, n.right)
            self.emit(_BINOPS[type(n.op)])
        elif isinstance(n, ast.UnaryOp):
            if isinstance(n.op, ast.USub):
                self.lower(expr, n.operand)
                self.emit(NEG)
            elif isinstance(n.op, ast.Not):
                self.lower(expr, n.operand)
                self.emit(NOT)
            else:
                self.bad(expr, n, "unsupported operator")
        elif isinstance(n, ast.Compare):
            if len(n.ops) != 1:
                self.bad(expr, n, "chained comparisons are not allowed")
            if type(n.ops[0]) not in _CMPOPS:
                self.bad(expr, n, "unsupported comparison")
            self.lower(expr, n.left)
            self.lower(expr, n.comparators[0])
            self.emit(_CMPOPS[type(n.ops[0])])
        elif isinstance(n, ast.BoolOp):
            op = AND if isinstance(n.op, ast.And) else OR
            self.lower(expr, n.values[0])
            for v in n.values[1:]:
                self.lower(expr, v)
                self.emit(op)
        elif isinstance(n, ast.Call):
            if not isinstance(n.func, ast.Name) or n.keywords:
                self.bad(expr, n, "unsupported call")
            f = n.func.id
            if f == "clamp":
                if len(n.args) != 3:
                    self.bad(expr, n, "clamp takes 3 arguments")
                x, lo, hi = n.args
                self.lower(expr, x)
                self.lower(expr, lo)
                self.emit(MAX)
                self.lower(expr, hi)
                self.emit(MIN)
            elif f in _CALLS:
                nargs, ops = _CALLS[f]
                if len(n.args) != nargs or any(isinstance(a, ast.Starred) for a in n.args):
                    self.bad(expr, n, f"{f} takes {nargs} argument{'s' if nargs > 1 else ''}")
                for a in n.args:
                    self.lower(expr, a)
                for o in ops:
                    self.emit(o)
            else:
                self.bad(expr, n, "unknown function")
        else:
            self.bad(expr, n, "unsupported syntax")


def compile_exprs(exprs: Sequence[str], nbands: int) -> Program:
    """One expression per output band, lowered into one program that ends each expression with ``STORE k``.
    ``ValueError`` naming the offending text for anything outside the whitelist, and for a program outside the limits
    (128 words, 32 constants, 8 outputs, stack depth 8)."""
    if isinstance(exprs, str):
        exprs = [exprs]
    exprs = list(exprs)
    if not 1 <= len(exprs) <= MAX_OUT:
        raise ValueError(f"{len(exprs)} expressions outside 1 ... {MAX_OUT} (one per output band)")
    low = _Lowering(int(nbands))
    for k, expr in enumerate(exprs):
        if not isinstance(expr, str):
            raise ValueError(f"expression {k} is not a string")
        try:
            tree = ast.parse(expr.strip(), mode="eval")
        except (SyntaxError, ValueError, RecursionError, MemoryError) as e:
            raise ValueError(f"cannot parse {expr!r}: {e}") from None
        try:
            low.lower(expr.strip(), tree.body)
        except RecursionError:
            raise ValueError(f"expression too deep: {expr!r}") from None
        low.emit(STORE, k)
        if len(low.code) > MAX_CODE:
            raise ValueError(f"program of more than {MAX_CODE} words at {expr!r}")
    prog = Program(np.array(low.code, np.uint16), np.array(low.consts, np.float64), len(exprs))
    try:
        validate(prog, int(nbands))
    except ValueError as e:
        raise ValueError(f"{e} in {exprs!r}") from None
    return prog


_QNAN = np.uint64(0x7FF8000000000000).view(np.float64)


def convert(v: np.ndarray, out_dtype) -> np.ndarray:
    """An f64 array in ``out_dtype`` by the rule's conversion."""
    dt = np.dtype(out_dtype)
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        if dt.kind == "f":
            return np.where(np.isnan(v), _QNAN, v).astype(dt)
        info = np.iinfo(dt)
        r = np.rint(v)
        r = np.where(np.isnan(r), 0.0, r)
        r = np.where(r < float(info.min), float(info.min), np.where(r > float(info.max), float(info.max), r))
        return r.astype(np.int64).astype(dt)


def default_fill(out_dtype) -> float:
    """NaN for float outputs, 0 for integer ones."""
    return float("nan") if np.dtype(out_dtype).kind == "f" else 0.0


def calc_arrays(raster: np.ndarray, program: Program, out_dtype, nodata: Optional[float] = None,
                fill: float = float("nan")) -> Tuple[np.ndarray, np.ndarray]:
    """The program over a ``(B, h, w)`` raster, op by op on f64 arrays: ``(the (nout, h, w) result in out_dtype, the
    per-output count of left-out pixels (uint64))``."""
    a = np.asarray(raster)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3:
        raise ValueError("raster must be (B, h, w) or (h, w)")
    dt = np.dtype(out_dtype)
    if dt.name not in DTYPES:
        raise TypeError(f"unsupported output dtype {dt}")
    B, h, w = a.shape
    validate(program, B)
    one, zero = np.float64(1.0), np.float64(0.0)
    left = np.zeros((h, w), bool)
    if nodata is not None:
        nd = np.float64(nodata)
        for b in program.bands_read():
            x = a[b].astype(np.float64)
            left |= np.isnan(x) | (x == nd)
    out = np.zeros((program.nout, h, w), dt)
    stack: List[np.ndarray] = []
    with np.errstate(all="ignore"):
        for op, arg in program.words():
            if op == CONST:
                stack.append(np.full((h, w), program.consts[arg], np.float64))
            elif op == BAND:
                stack.append(a[arg].astype(np.float64))
            elif op == STORE:
                v = stack.pop()
                out[arg] = convert(np.where(left, np.float64(fill), v), dt)
            elif op in _UNARY:
                x = stack.pop()
                if op == NEG:
                    r = -x
                elif op == ABS:
                    r = np.abs(x)
                elif op == SQRT:
                    r = np.sqrt(x)
                elif op == FLOOR:
                    r = np.floor(x)
                else:
                    r = np.where(x != 0.0, zero, one)
                stack.append(r)
            elif op == SELECT:
                y = stack.pop()
                x = stack.pop()
                c = stack.pop()
                stack.append(np.where(c != 0.0, x, y))
            else:
                y = stack.pop()
                x = stack.pop()
                if op == ADD:
                    r = x + y
                elif op == SUB:
                    r = x - y
                elif op == MUL:
                    r = x * y
                elif op == DIV:
                    r = x / y
                elif op == MIN:
                    r = np.where(x < y, x, y)
                elif op == MAX:
                    r = np.where(x > y, x, y)
                elif op == AND:
                    r = np.where((x != 0.0) & (y != 0.0), one, zero)
                elif op == OR:
                    r = np.where((x != 0.0) | (y != 0.0), one, zero)
                else:
                    c = {LT: x < y, LE: x <= y, GT: x > y, GE: x >= y, EQ: x == y, NE: x != y}[op]
                    r = np.where(c, one, zero)
                stack.append(r)
    counts = np.full(program.nout, np.count_nonzero(left), np.uint64)
    return out, counts
