"""Filter expressions: legacy string-DSL parsing, evaluation, pruning.

Implements the reference's Java filter string DSL
(``rust/lakesoul-io/src/filter/parser.rs:52-120``):
``and(l,r) or(l,r) not(e) eq(col,v) noteq(col,v) gt/gteq/lt/lteq(col,v)``
with ``null`` literals for is-null tests; plus python tuple filters
``(col, op, value)``. Beyond the reference: ``in`` and the pattern
predicates ``like notlike startswith endswith contains`` on string and
binary columns (``Like``), evaluated by the string-predicate kernel
(csrc/hip/str_pred.hip) or its host twin (csrc/cpp/str_pred.h).

The same expression drives three stages, mirroring the reference's
filter classification (session.rs:760-791):
1. partition pruning (range-partition columns vs partition_desc),
2. file/row-group pruning from parquet min/max statistics,
3. exact row-level evaluation on decoded batches (torch masks, GPU or CPU).
"""

from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from .schema import Schema


class Expr:
    def evaluate(self, batch) -> torch.Tensor:  # bool mask
        raise NotImplementedError

    def prune_stats(self, stats: Dict[str, Tuple]) -> bool:
        """False = no row can match (skip the file/row group)."""
        return True

    def partition_prune(self, part_values: Dict[str, str]) -> bool:
        """False = partition cannot match."""
        return True

    def pk_eq_values(self) -> Dict[str, object]:
        """col -> constant for top-level AND-ed equality predicates."""
        return {}

    def __getstate__(self):
        # compiled string operands (host and device tensors) stay behind
        # when an expression is copied or sent to another process
        d = dict(self.__dict__)
        d.pop("_operands", None)
        return d

    def columns(self) -> set:
        """All column names referenced by this expression."""
        out = set()
        for f in getattr(self, "__dataclass_fields__", {}):
            v = getattr(self, f)
            if isinstance(v, Expr):
                out |= v.columns()
        if hasattr(self, "col"):
            out.add(self.col)
        return out


@dataclass
class Literal(Expr):
    value: bool

    def evaluate(self, batch):
        n = batch.num_rows
        dev = _batch_device(batch)
        return torch.full((n,), self.value, dtype=torch.bool, device=dev)

    def prune_stats(self, stats):
        return self.value

    def partition_prune(self, pv):
        return self.value


@dataclass
class And(Expr):
    left: Expr
    right: Expr

    def evaluate(self, batch):
        return self.left.evaluate(batch) & self.right.evaluate(batch)

    def prune_stats(self, stats):
        return self.left.prune_stats(stats) and self.right.prune_stats(stats)

    def partition_prune(self, pv):
        return self.left.partition_prune(pv) and self.right.partition_prune(pv)

    def pk_eq_values(self):
        d = dict(self.left.pk_eq_values())
        d.update(self.right.pk_eq_values())
        return d


@dataclass
class Or(Expr):
    left: Expr
    right: Expr

    def evaluate(self, batch):
        return self.left.evaluate(batch) | self.right.evaluate(batch)

    def prune_stats(self, stats):
        return self.left.prune_stats(stats) or self.right.prune_stats(stats)

    def partition_prune(self, pv):
        return self.left.partition_prune(pv) or self.right.partition_prune(pv)


@dataclass
class Not(Expr):
    inner: Expr

    def evaluate(self, batch):
        return ~self.inner.evaluate(batch)


@dataclass
class IsNull(Expr):
    col: str
    negate: bool = False

    def evaluate(self, batch):
        c = batch.columns[self.col]
        n = batch.num_rows
        dev = _batch_device(batch)
        if c.validity is None:
            m = torch.zeros(n, dtype=torch.bool, device=dev)
        else:
            m = ~(c.validity.to(torch.bool))
        return ~m if self.negate else m

    def partition_prune(self, pv):
        if self.col not in pv:
            return True
        is_null = pv[self.col] is None
        return (not is_null) if self.negate else is_null


@dataclass
class Cmp(Expr):
    col: str
    op: str  # eq noteq gt gteq lt lteq in
    value: object

    def evaluate(self, batch):
        c = batch.columns[self.col]
        n = batch.num_rows
        if c.is_string:
            # validity is fused into the kernel's mask
            return _str_pred_mask(self, ("cmp", self.op), self._compile, c,
                                  _str_op(self.op))
        else:
            t = c.data
            v = self.value
            if c.dtype.startswith("decimal") and not isinstance(v, (list, tuple, set)):
                # logical literal -> unscaled int64 (decimal columns store
                # unscaled values; exact scaling via decimal module)
                import decimal as _dec

                from .schema import decimal_params

                _, sc = decimal_params(c.dtype)
                v = int(_dec.Decimal(str(v)).scaleb(sc).to_integral_value())
            if self.op == "eq":
                out = t == v
            elif self.op == "noteq":
                out = t != v
            elif self.op == "gt":
                out = t > v
            elif self.op == "gteq":
                out = t >= v
            elif self.op == "lt":
                out = t < v
            elif self.op == "lteq":
                out = t <= v
            elif self.op == "in":
                out = torch.isin(t, torch.tensor(list(v), device=t.device))
            else:
                raise ValueError(self.op)
        if c.validity is not None:
            out = out & c.validity.to(torch.bool)
        return out

    def _compile(self):
        from ..ops import cpp

        if self.op == "in":
            if isinstance(self.value, (str, bytes, bytearray, memoryview)):
                raise TypeError("'in' on a string column takes a collection of literals")
            return cpp().str_pred_compile_set([_lit_bytes(x) for x in self.value])
        return cpp().str_pred_compile_literal(_lit_bytes(self.value))

    def prune_stats(self, stats):
        if self.col not in stats:
            return True
        mn, mx = stats[self.col]
        if mn is None or mx is None:
            return True
        v = self.value
        try:
            if self.op == "eq":
                return mn <= v <= mx
            if self.op == "gt":
                return mx > v
            if self.op == "gteq":
                return mx >= v
            if self.op == "lt":
                return mn < v
            if self.op == "lteq":
                return mn <= v
            if self.op == "in":
                return any(mn <= x <= mx for x in v)
        except TypeError:
            return True
        return True

    def partition_prune(self, pv):
        if self.col not in pv:
            return True
        if pv[self.col] is None:
            # NULL partition value: comparisons are unknown -> no row of
            # this partition can satisfy the predicate
            return False
        if self.op == "in":
            # the partition value against each literal, in the literal's type
            try:
                return any(
                    (pv[self.col] if isinstance(x, str) else type(x)(pv[self.col])) == x
                    for x in self.value)
            except (TypeError, ValueError):
                return True
        try:
            col_v = type(self.value)(pv[self.col]) if not isinstance(self.value, str) else pv[self.col]
        except (TypeError, ValueError):
            return True
        return _cmp_py(col_v, self.op, self.value)

    def pk_eq_values(self):
        return {self.col: self.value} if self.op == "eq" else {}


@dataclass
class Like(Expr):
    """SQL LIKE on a string or binary column. ``%`` matches any run of
    bytes, ``_`` one character (a UTF-8 code point for ``string``, a byte
    for ``binary``); ``escape`` makes the next ``%``, ``_`` or escape
    character literal. A NULL row is False, also when negated."""
    col: str
    pattern: object
    negate: bool = False
    escape: str = "\\"

    def evaluate(self, batch):
        c = batch.columns[self.col]
        if not c.is_string:
            raise TypeError(f"LIKE needs a string or binary column, {self.col} is {c.dtype}")
        utf8 = c.dtype != "binary"
        return _str_pred_mask(self, ("like", utf8), lambda: self._compile(utf8), c,
                              _OP_NOT_LIKE if self.negate else _OP_LIKE)

    def _escape_byte(self) -> int:
        e = _lit_bytes(self.escape) if self.escape else b""
        if len(e) > 1:
            raise ValueError("LIKE escape must be one byte")
        return e[0] if e else -1

    def _compile(self, utf8: bool):
        from ..ops import cpp

        return cpp().str_pred_compile_like(_lit_bytes(self.pattern),
                                           self._escape_byte(), utf8)

    def _match_one(self, value, utf8: bool = True) -> bool:
        """The pattern on one value (None is NULL), through the host twin."""
        if value is None:
            return False
        v = _lit_bytes(value)
        col = _OneValue(torch.tensor([0, len(v)], dtype=torch.int32),
                        torch.frombuffer(bytearray(v), dtype=torch.uint8)
                        if v else torch.empty(0, dtype=torch.uint8))
        m = _str_pred_mask(self, ("like", utf8), lambda: self._compile(utf8), col,
                           _OP_NOT_LIKE if self.negate else _OP_LIKE)
        return bool(m[0])

    def literal_prefix(self) -> bytes:
        """The literal bytes in front of the pattern's first wildcard."""
        pat, esc = _lit_bytes(self.pattern), self._escape_byte()
        out = bytearray()
        i = 0
        while i < len(pat):
            b = pat[i]
            if b == esc:
                if i + 1 < len(pat):
                    i += 1
                out.append(pat[i])
            elif b in b"%_":
                break
            else:
                out.append(b)
            i += 1
        return bytes(out)

    def prune_stats(self, stats):
        if self.negate or self.col not in stats:
            return True
        mn, mx = stats[self.col]
        p = self.literal_prefix()
        if mn is None or mx is None or not p:
            return True
        try:
            if isinstance(mn, str):
                if "\ufffd" in mn or "\ufffd" in mx:
                    return True      # statistics that were no UTF-8: their order is lost
                p = p.decode("utf-8")
            return mn[:len(p)] <= p <= mx[:len(p)]
        except (TypeError, UnicodeDecodeError):
            return True

    def partition_prune(self, pv):
        if self.col not in pv:
            return True
        if pv[self.col] is None:
            return False
        try:
            return self._match_one(pv[self.col])
        except TypeError:
            return True


@dataclass
class _OneValue:
    offsets: torch.Tensor
    bytes_: torch.Tensor
    validity: Optional[torch.Tensor] = None


_STR_OP_NAMES = ("eq", "noteq", "lt", "lteq", "gt", "gteq", "in")
_OP_LIKE, _OP_NOT_LIKE = 7, 8


def _str_op(op: str) -> int:
    if op not in _STR_OP_NAMES:
        raise ValueError(op)
    return _STR_OP_NAMES.index(op)


def _lit_bytes(v) -> bytes:
    if isinstance(v, str):
        return v.encode("utf-8")
    if isinstance(v, (bytes, bytearray, memoryview, np.bytes_)):
        return bytes(v)
    raise TypeError(f"string predicate literal must be str or bytes, not {type(v).__name__}")


def _to_device(t: torch.Tensor, dev) -> torch.Tensor:
    """Host operand -> device without a host sync: from pinned memory,
    asynchronously (the pinned block is kept until the copy has run)."""
    try:
        return t.pin_memory().to(dev, non_blocking=True)
    except RuntimeError:
        return t.to(dev)


def _str_pred_mask(owner: Expr, key, compile_fn, c, op: int) -> torch.Tensor:
    """One leaf predicate over string column ``c`` -> bool mask, validity
    included. The compiled operand is made once per expression and kept on
    it, per device."""
    from ..ops import cpp, hip

    cache = owner.__dict__.setdefault("_operands", {})
    host = cache.get(key)
    if host is None:
        host = cache[key] = tuple(compile_fn())
    dev = c.offsets.device
    offsets = c.offsets if c.offsets.is_contiguous() else c.offsets.contiguous()
    if dev.type != "cuda":
        return cpp().str_pred_mask(offsets, c.bytes_, c.validity, op, host[0], host[1])
    on_dev = cache.get((key, dev))
    if on_dev is None:
        on_dev = cache[(key, dev)] = tuple(_to_device(t, dev) for t in host)
    bytes_ = c.bytes_ if c.bytes_.is_contiguous() else c.bytes_.contiguous()
    # a pattern whose segments are all anchored searches for nothing: a
    # thread per row whatever the value length (the binding picks otherwise)
    shape = None
    if op >= _OP_LIKE:
        flags, nseg = int(host[1][0]), int(host[1][1])
        if nseg - (flags & 1) - ((flags >> 1) & 1) <= 0:
            shape = "rows"
    return hip().str_pred_mask(offsets, bytes_, c.validity, op, on_dev[0], on_dev[1],
                               shape=shape)


def _cmp_py(a, op, b) -> bool:
    if op == "eq":
        return a == b
    if op == "noteq":
        return a != b
    if op == "gt":
        return a > b
    if op == "gteq":
        return a >= b
    if op == "lt":
        return a < b
    if op == "lteq":
        return a <= b
    if op == "in":
        return a in b
    raise ValueError(op)


def _batch_device(batch):
    for c in batch.columns.values():
        t = c.data if not c.is_string else c.bytes_
        if t is not None:
            return t.device
    return torch.device("cpu")


_TUPLE_OPS = {
    "==": "eq", "=": "eq", "!=": "noteq", ">": "gt", ">=": "gteq",
    "<": "lt", "<=": "lteq", "in": "in",
    "eq": "eq", "noteq": "noteq", "gt": "gt", "gteq": "gteq",
    "lt": "lt", "lteq": "lteq",
}


def escape_like(literal, escape: str = "\\"):
    """``literal`` with every ``%``, ``_`` and escape character escaped."""
    if isinstance(literal, str):
        return "".join(escape + ch if ch in ("%", "_", escape) else ch for ch in literal)
    esc = escape.encode()
    return b"".join(esc + bytes([b]) if bytes([b]) in (b"%", b"_", esc) else bytes([b])
                    for b in _lit_bytes(literal))


def pattern_expr(col: str, op: str, literal) -> "Like":
    """like / not like / starts_with / ends_with / contains as a Like."""
    op = op.lower().replace("_", "").replace(" ", "")
    if op in ("like", "notlike"):
        return Like(col, literal, negate=(op == "notlike"))
    pct = "%" if isinstance(literal, str) else b"%"
    lit = escape_like(literal)
    if op == "startswith":
        return Like(col, lit + pct)
    if op == "endswith":
        return Like(col, pct + lit)
    if op == "contains":
        return Like(col, pct + lit + pct)
    raise ValueError(f"unknown pattern op {op}")


_PATTERN_OPS = ("like", "notlike", "startswith", "endswith", "contains")


def from_tuples(filters: List[Tuple], schema: Schema) -> Optional[Expr]:
    expr: Optional[Expr] = None
    for col, op, val in filters:
        e: Expr
        if op not in _TUPLE_OPS and isinstance(op, str) and \
                op.lower().replace("_", "").replace(" ", "") in _PATTERN_OPS:
            e = pattern_expr(col, op, val)
        else:
            e = Cmp(col, _TUPLE_OPS[op], val)
        expr = e if expr is None else And(expr, e)
    return expr


def parse_filter_dsl(s: str, schema: Schema) -> Expr:
    """Parse the reference's Java filter string DSL (parser.rs:52-120)."""
    s = s.strip()
    i = s.find("(")
    if i < 0 or not s.endswith(")"):
        raise ValueError(f"bad filter string: {s}")
    op = s[:i].strip()
    body = s[i + 1 : -1]
    # split top-level comma
    k = 0
    split = -1
    for j, ch in enumerate(body):
        if ch == "(":
            k += 1
        elif ch == ")":
            k -= 1
        elif ch == "," and k == 0 and split < 0:
            split = j
    if op == "not":
        return Not(parse_filter_dsl(body, schema))
    if op in ("and", "or"):
        left, right = body[:split], body[split + 1 :]
        l, r = parse_filter_dsl(left, schema), parse_filter_dsl(right, schema)
        return And(l, r) if op == "and" else Or(l, r)
    if op in ("eq", "noteq", "gt", "gteq", "lt", "lteq"):
        col = body[:split].strip()
        rhs = body[split + 1 :].strip()
        if rhs == "null":
            if op == "eq":
                return IsNull(col)
            if op == "noteq":
                return IsNull(col, negate=True)
            return Literal(True)
        try:
            f = schema.field(col)
        except KeyError:
            return Literal(False)
        return Cmp(col, op, _parse_literal(rhs, f.dtype))
    if op in _PATTERN_OPS:
        # an extension: the reference's DSL has no pattern ops
        col = body[:split].strip()
        rhs = body[split + 1 :].strip()
        try:
            f = schema.field(col)
        except KeyError:
            return Literal(False)
        if f.dtype not in ("string", "binary"):
            raise ValueError(f"{op} needs a string column, {col} is {f.dtype}")
        return pattern_expr(col, op, _parse_literal(rhs, f.dtype))
    raise ValueError(f"unknown filter op {op}")


def _parse_literal(s: str, dtype: str):
    if dtype.startswith("decimal"):
        return float(s)   # scaled at evaluate() against the unscaled column
    if dtype in ("string", "binary"):
        if len(s) >= 2 and s[0] == s[-1] and s[0] in "'\"":
            s = s[1:-1]
        return s
    if dtype in ("float32", "float64"):
        return float(s)
    if dtype == "bool":
        return s.lower() in ("true", "1")
    return int(s)


def resolve_filters(filters, schema: Schema) -> Optional[Expr]:
    """Accept None | Expr | DSL string | list of (col,op,val) tuples |
    Substrait protobuf bytes (Plan or ExtendedExpression — the encodings
    engines push through the C ABI, reference parser.rs:44-60)."""
    if filters is None:
        return None
    if isinstance(filters, Expr):
        return filters
    if isinstance(filters, (bytes, bytearray, memoryview)):
        from .substrait import decode_substrait_filter

        return decode_substrait_filter(bytes(filters), schema)
    if isinstance(filters, str):
        return parse_filter_dsl(filters, schema)
    if isinstance(filters, (list, tuple)):
        if not filters:
            return None
        return from_tuples(list(filters), schema)
    raise TypeError(f"unsupported filters: {filters!r}")


def decode_stat(raw: bytes, dtype: str):
    if raw is None:
        return None
    if dtype in ("int32", "int8", "int16", "date32"):
        return struct.unpack("<i", raw)[0]
    if dtype in ("int64", "timestamp[us]", "timestamp[ms]", "timestamp[ns]"):
        return struct.unpack("<q", raw)[0]
    if dtype == "float32":
        return struct.unpack("<f", raw)[0]
    if dtype == "float64":
        return struct.unpack("<d", raw)[0]
    if dtype == "string":
        return raw.decode("utf-8", "replace")
    if dtype == "binary":
        return raw
    return None
