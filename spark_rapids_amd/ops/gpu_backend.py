"""GPU backend: drives the hipdf CDNA4 kernels over device Columns.

Buffers live in the PyTorch-ROCm caching allocator (the RMM-style pool);
every columnar computation below is a hand-written HIP kernel from
native/hipdf — torch is used only for allocation, D2H/H2D movement and
byte-level cat/zero (memcpy/memset-class work). If the native extension is
missing this module fails to import and ops.backend_for raises — there is
no silent eager fallback on GPU.
"""
from __future__ import annotations

import struct
from typing import List, Optional, Tuple

import numpy as np
import torch

from ..column import (Column, ColumnBatch, DictColumn, mask_nbytes,
                      torch_dtype)
from ..types import DType, TypeId
from .cpu_backend import (SEQUENCE_ERROR, SEQUENCE_OVERFLOW,
                          SLICE_LENGTH_ERROR, SLICE_START_ERROR,
                          _same_type_operands, _sequence_operands)

import importlib


def _load_ext():
    try:
        return importlib.import_module("hipdf")
    except ImportError as e:
        raise ImportError(
            "hipdf native extension not built; run python native/hipdf/build.py"
        ) from e


ext = _load_ext()

# ---------------------------------------------------------------------------
# enums shared with the kernels
# ---------------------------------------------------------------------------
_HT = {
    TypeId.BOOL: 0, TypeId.INT8: 1, TypeId.INT16: 2, TypeId.INT32: 3,
    TypeId.DATE32: 3, TypeId.INT64: 4, TypeId.TIMESTAMP: 4,
    TypeId.DECIMAL64: 4, TypeId.FLOAT32: 5, TypeId.FLOAT64: 6,
}
_BIN_OPS = {
    "add": 0, "sub": 1, "mul": 2, "div": 3, "int_div": 4, "mod": 5,
    "pmod": 6, "pow": 7, "eq": 8, "ne": 9, "lt": 10, "le": 11, "gt": 12,
    "ge": 13, "eq_null_safe": 14, "and": 15, "or": 16, "bitand": 17,
    "bitor": 18, "bitxor": 19, "shiftleft": 20, "shiftright": 21,
    "min": 22, "max": 23, "round": 24,
}
_CMP_OPS = {"eq", "ne", "lt", "le", "gt", "ge", "eq_null_safe"}
_BOOL_OPS = {"and", "or"}
_NULL_PRODUCING = {"div", "int_div", "mod", "pmod"}
_UN_OPS = {
    "neg": 0, "abs": 1, "not": 2, "sqrt": 3, "exp": 4, "log": 5, "floor": 6,
    "ceil": 7, "sin": 8, "cos": 9, "tan": 10, "is_nan": 11, "year": 12,
    "month": 13, "day": 14,
}
_HK_INT, _HK_LONG, _HK_FLOAT, _HK_DOUBLE = 0, 1, 2, 3
_RED = {"sum": 0, "min": 1, "max": 2, "count": 3}
_GB = {"sum": 0, "min": 1, "max": 2, "count": 3, "count_all": 4,
       "first": 5, "last": 5, "bit_and": 6, "bit_or": 7, "bit_xor": 8}
_JOIN = {"inner": 0, "left": 1, "semi": 2, "anti": 3, "full": 4}





def _stream() -> int:
    # follow torch's CURRENT stream: the prefetch pool decodes files on
    # side streams (with torch.cuda.stream(...)) to overlap H2D + decode
    # with main-stream compute, so hipdf kernels must land on whatever
    # stream the calling thread has current
    return torch.cuda.current_stream().cuda_stream


def set_stream(handle: Optional[int]) -> None:
    # retained for API compatibility: _stream() now always follows
    # torch.cuda.current_stream(), which set_stream callers control via
    # `with torch.cuda.stream(...)`
    del handle


def _ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _ht(dt: DType) -> int:
    return _HT[dt.id]


def _alloc(n: int, dt: DType) -> torch.Tensor:
    words = 2 * n if dt.id is TypeId.DECIMAL128 else n
    if words == 0:
        return torch.empty(1, dtype=torch_dtype(dt), device="cuda")[:0]
    return torch.empty(words, dtype=torch_dtype(dt), device="cuda")


def _alloc_mask(n: int) -> torch.Tensor:
    return torch.empty(mask_nbytes(n), dtype=torch.uint8, device="cuda")


def _empty_col(dtype: DType) -> Column:
    if dtype.id is TypeId.STRING:
        return Column(dtype, 0, torch.zeros(0, dtype=torch.uint8, device="cuda"),
                      None, torch.zeros(1, dtype=torch.int32, device="cuda"), 0)
    if dtype.id is TypeId.STRUCT:
        return Column(dtype, 0,
                      torch.zeros(0, dtype=torch.uint8, device="cuda"),
                      None, None, 0,
                      tuple(_empty_col(c) for c in dtype.children))
    return Column(dtype, 0, torch.zeros(0, dtype=torch_dtype(dtype),
                                        device="cuda"), None, None, 0)


_I128_ARITH = {"add": 0, "sub": 1, "min": 22, "max": 23}


# ---------------------------------------------------------------------------
# elementwise
# ---------------------------------------------------------------------------

def binary_op(op: str, lhs: Column, rhs: Column, out_dtype: DType) -> Column:
    return _binary(op, lhs, rhs, None, out_dtype)


def binary_op_scalar(op: str, lhs: Column, scalar, out_dtype: DType) -> Column:
    return _binary(op, lhs, None, scalar, out_dtype)


_STR_CMP = {"eq": 0, "ne": 1, "lt": 2, "le": 3, "gt": 4, "ge": 5}


def decimal_mul_div(op: str, lhs: Column, rhs: Column,
                    out_dtype: DType) -> Column:
    """Exact decimal multiply/divide on device. dec64 operands ride
    k_dec64_mul_div (__int128 intermediates); any decimal128 operand
    routes to k_dec_mul_div_wide (256-bit product / u192-remainder long
    division). NULL on div-by-zero / overflow."""
    n = lhs.size
    s = _stream()
    s1, s2, st = lhs.dtype.scale, rhs.dtype.scale, out_dtype.scale
    shift = (s1 + s2 - st) if op == "mul" else (st + s2 - s1)
    is128 = out_dtype.id is TypeId.DECIMAL128
    width = 2 * n if is128 else n
    out = torch.empty(max(width, 1), dtype=torch.int64,
                      device="cuda")[:width]
    ov = _alloc_mask(n)
    a128 = lhs.dtype.id is TypeId.DECIMAL128
    b128 = rhs.dtype.id is TypeId.DECIMAL128
    if n and not (a128 or b128):
        ext.dec64_mul_div(1 if op == "div" else 0, lhs.data.data_ptr(),
                          rhs.data.data_ptr(), _ptr(lhs.validity),
                          _ptr(rhs.validity), out.data_ptr(), ov.data_ptr(),
                          1 if is128 else 0, shift, out_dtype.precision,
                          n, s)
    elif n:
        ext.dec_mul_div_wide(1 if op == "div" else 0, lhs.data.data_ptr(),
                             rhs.data.data_ptr(), _ptr(lhs.validity),
                             _ptr(rhs.validity), 1 if a128 else 0,
                             1 if b128 else 0, out.data_ptr(),
                             ov.data_ptr(), 1 if is128 else 0, shift,
                             out_dtype.precision, n, s)
    return Column(out_dtype, n, out, ov, null_count=None)


def _binary(op, lhs: Column, rhs: Optional[Column], scalar, out_dtype) -> Column:
    n = lhs.size
    s = _stream()
    scalar_rhs = rhs is None
    if lhs.dtype.id is TypeId.STRING:
        if op == "concat" and not scalar_rhs:
            return str_concat(lhs, rhs)
        if op not in _STR_CMP:
            raise NotImplementedError(f"string op {op} not on GPU")
        out = _alloc(n, out_dtype)
        if scalar_rhs:
            pat = _pattern_tensor(scalar)
            ext.str_cmp_scalar(_STR_CMP[op], lhs.offsets.data_ptr(),
                               lhs.data.data_ptr(), pat.data_ptr(),
                               pat.numel(), out.data_ptr(), n, s)
            v = lhs.validity.clone() if lhs.validity is not None else None
            return Column(out_dtype, n, out, v, null_count=lhs._null_count)
        ext.str_cmp(_STR_CMP[op], lhs.offsets.data_ptr(), lhs.data.data_ptr(),
                    rhs.offsets.data_ptr(), rhs.data.data_ptr(),
                    out.data_ptr(), n, s)
        # combine validities via the bool AND kernel on expanded masks
        return _with_and_validity(out, lhs, rhs, out_dtype, n, s)
    if lhs.dtype.id is TypeId.DECIMAL128:
        if scalar_rhs:
            raise NotImplementedError("decimal128 scalar ops not on GPU")
        ov = _alloc_mask(n)
        if op in _I128_ARITH and op in ("add", "sub", "min", "max"):
            out = _alloc(n, out_dtype)
            ext.i128_arith(_I128_ARITH[op], lhs.data.data_ptr(),
                           rhs.data.data_ptr(), _ptr(lhs.validity),
                           _ptr(rhs.validity), out.data_ptr(), ov.data_ptr(),
                           n, s)
            return Column(out_dtype, n, out, ov, null_count=None)
        if op in _STR_CMP:
            out = _alloc(n, out_dtype)
            ext.i128_cmp(_STR_CMP[op], lhs.data.data_ptr(),
                         rhs.data.data_ptr(), _ptr(lhs.validity),
                         _ptr(rhs.validity), out.data_ptr(), ov.data_ptr(),
                         n, s)
            has_valid = lhs.validity is not None or rhs.validity is not None
            return Column(out_dtype, n, out, ov if has_valid else None,
                          null_count=None if has_valid else 0)
        raise NotImplementedError(f"decimal128 op {op} not on GPU")
    t = _ht(lhs.dtype)
    sd, si = 0.0, 0
    if scalar_rhs and scalar is not None:
        if lhs.dtype.is_floating:
            sd = float(scalar)
        else:
            si = int(scalar)
    av = _ptr(lhs.validity)
    bv = 0 if scalar_rhs else _ptr(rhs.validity)
    has_in_valid = lhs.validity is not None or (not scalar_rhs and rhs.validity is not None)

    if op in _BOOL_OPS:
        out = _alloc(n, out_dtype)
        ov = _alloc_mask(n)  # Kleene output can always carry nulls
        ext.binary_bool(_BIN_OPS[op], lhs.data.data_ptr(),
                        0 if scalar_rhs else rhs.data.data_ptr(),
                        int(bool(si or sd)) if scalar_rhs else 0, scalar_rhs,
                        av, bv, out.data_ptr(), ov.data_ptr(), n, s)
        if not has_in_valid:
            return Column(out_dtype, n, out, None, null_count=0)
        return Column(out_dtype, n, out, ov, null_count=None)
    if op in _CMP_OPS:
        out = _alloc(n, out_dtype)
        need_mask = has_in_valid and op != "eq_null_safe"
        ov = _alloc_mask(n) if need_mask else None
        ext.binary_cmp(_BIN_OPS[op], t, lhs.data.data_ptr(),
                       0 if scalar_rhs else rhs.data.data_ptr(), sd, si,
                       scalar_rhs, av, bv, out.data_ptr(), _ptr(ov), n, s)
        return Column(out_dtype, n, out, ov,
                      null_count=None if need_mask else 0)
    out = _alloc(n, out_dtype)
    need_mask = has_in_valid or op in _NULL_PRODUCING
    ov = _alloc_mask(n) if need_mask else None
    ext.binary_arith(_BIN_OPS[op], t, lhs.data.data_ptr(),
                     0 if scalar_rhs else rhs.data.data_ptr(), sd, si,
                     scalar_rhs, av, bv, out.data_ptr(), _ptr(ov), n, s)
    return Column(out_dtype, n, out, ov, null_count=None if need_mask else 0)


def _pattern_tensor(pattern) -> torch.Tensor:
    b = str(pattern).encode("utf-8")
    if not b:
        return torch.zeros(1, dtype=torch.uint8, device="cuda")[:0]
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _and_masks(a: Optional[torch.Tensor], b: Optional[torch.Tensor]):
    if a is None:
        return b.clone() if b is not None else None
    if b is None:
        return a.clone()
    n = min(a.numel(), b.numel())
    return (a[:n].view(torch.int32) & b[:n].view(torch.int32)).view(torch.uint8)


def _with_and_validity(out, lhs, rhs, out_dtype, n, s):
    v = _and_masks(lhs.validity, rhs.validity)
    return Column(out_dtype, n, out, v,
                  null_count=None if v is not None else 0)


def str_predicate(op: str, col: Column, pattern: str) -> Column:
    n = col.size
    s = _stream()
    out = _alloc(n, DType.bool_())
    if op == "rlike":
        from .regex_compiler import compile_regex

        prog = compile_regex(pattern)  # tagger pre-checks; raise = bug
        flat = []
        for o, a0, a1 in prog.ops:
            flat.extend([o, a0, a1])
        prog_t = torch.tensor(flat, dtype=torch.int32).cuda()
        cls_blob = b"".join(prog.classes) or b"\x00" * 32
        cls_t = torch.frombuffer(bytearray(cls_blob),
                                 dtype=torch.uint8).cuda()
        overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
        ext.regex_match(prog_t.data_ptr(), len(prog.ops), cls_t.data_ptr(),
                        col.offsets.data_ptr(), col.data.data_ptr(),
                        out.data_ptr(), overflow.data_ptr(), n, s)
        if int(overflow.item()) > 0:
            # pathological backtracking: redo the whole column on CPU
            from . import cpu_backend

            host = cpu_backend.str_predicate(op, col.cpu(), pattern)
            return host.cuda()
        v = col.validity.clone() if col.validity is not None else None
        return Column(DType.bool_(), n, out, v, null_count=col._null_count)
    pat = _pattern_tensor(pattern)
    if op == "like":
        ext.str_like(col.offsets.data_ptr(), col.data.data_ptr(),
                     pat.data_ptr(), pat.numel(), out.data_ptr(), n, s)
    else:
        mode = {"contains": 0, "starts_with": 1, "ends_with": 2}[op]
        ext.str_find(mode, col.offsets.data_ptr(), col.data.data_ptr(),
                     pat.data_ptr(), pat.numel(), out.data_ptr(), n, s)
    v = col.validity.clone() if col.validity is not None else None
    return Column(DType.bool_(), n, out, v, null_count=col._null_count)


def _rx_prog_tensors(pattern: str):
    from .regex_compiler import compile_regex

    prog = compile_regex(pattern)
    flat = []
    for o, a0, a1 in prog.ops:
        flat.extend([o, a0, a1])
    prog_t = torch.tensor(flat, dtype=torch.int32).cuda()
    cls_blob = b"".join(prog.classes) or b"\x00" * 32
    cls_t = torch.frombuffer(bytearray(cls_blob), dtype=torch.uint8).cuda()
    return prog, prog_t, cls_t


def regexp_extract(col: Column, pattern: str, group: int) -> Column:
    n = col.size
    s = _stream()
    if n == 0:
        return _empty_col(DType.string())
    prog, prog_t, cls_t = _rx_prog_tensors(pattern)
    if group > prog.ngroups:
        raise ValueError(f"regexp_extract group {group} > "
                         f"{prog.ngroups} capture groups")
    starts = torch.empty(n, dtype=torch.int32, device="cuda")
    lens = torch.empty(n, dtype=torch.int64, device="cuda")
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    ext.regex_extract(prog_t.data_ptr(), len(prog.ops), cls_t.data_ptr(),
                      col.offsets.data_ptr(), col.data.data_ptr(), group,
                      starts.data_ptr(), lens.data_ptr(),
                      overflow.data_ptr(), n, s)
    if int(overflow.item()) > 0:
        from . import cpu_backend

        return cpu_backend.regexp_extract(col.cpu(), pattern, group).cuda()
    return _strings_from_spans(col, starts, lens, n, s)


def _strings_from_spans(col: Column, starts, lens, n, s) -> Column:
    """Assemble a string column from absolute (start, len) spans over the
    source bytes (substr_copy compaction)."""
    scanned, total = _exclusive_scan_i64(lens)
    out_bytes = torch.empty(max(total, 1), dtype=torch.uint8,
                            device="cuda")[:total]
    if total:
        ext.substr_copy(col.data.data_ptr(), starts.data_ptr(),
                        lens.data_ptr(), scanned.data_ptr(),
                        out_bytes.data_ptr(), n, s)
    offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), n, s)
    offs[n] = total
    v = col.validity.clone() if col.validity is not None else None
    return Column(DType.string(), n, out_bytes, v, offs,
                  null_count=col._null_count)


def _compile_replacement(replacement: str, ngroups: int):
    """Java appendReplacement template -> (ops int32 triples, literal
    bytes): $g group refs, backslash escapes."""
    ops_l = []
    lit = bytearray()
    cur = bytearray()

    def flush():
        nonlocal cur
        if cur:
            ops_l.append((0, len(lit), len(cur)))
            lit.extend(cur)
            cur = bytearray()

    i = 0
    while i < len(replacement):
        c = replacement[i]
        if c == "$" and i + 1 < len(replacement) and \
                replacement[i + 1].isdigit():
            g = int(replacement[i + 1])
            if g > ngroups:
                raise ValueError(f"replacement group ${g} out of range")
            flush()
            ops_l.append((1, g, 0))
            i += 2
        elif c == "\\" and i + 1 < len(replacement):
            cur.extend(replacement[i + 1].encode("utf-8"))
            i += 2
        else:
            cur.extend(c.encode("utf-8"))
            i += 1
    flush()
    return ops_l, bytes(lit)


def concat_ws(sep: str, cols) -> Column:
    n = cols[0].size
    s = _stream()
    if n == 0:
        return _empty_col(DType.string())
    # HipdfStrColDesc (see native/hipdf/include/hipdf.h)
    blob = b"".join(struct.pack("<qqq", c.offsets.data_ptr(),
                                c.data.data_ptr(), _ptr(c.validity))
                    for c in cols)
    desc = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    sep_t = _pattern_tensor(sep or "\x00")
    seplen = len(sep.encode("utf-8"))
    lens = torch.empty(n, dtype=torch.int64, device="cuda")
    ext.str_concat_ws(desc.data_ptr(), len(cols), sep_t.data_ptr(), seplen,
                      0, lens.data_ptr(), 0, 0, n, s)
    scanned, total = _exclusive_scan_i64(lens)
    out = torch.empty(max(total, 1), dtype=torch.uint8,
                      device="cuda")[:total]
    if total:
        ext.str_concat_ws(desc.data_ptr(), len(cols), sep_t.data_ptr(),
                          seplen, scanned.data_ptr(), lens.data_ptr(),
                          out.data_ptr(), 1, n, s)
    offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), n, s)
    offs[n] = total
    return Column(DType.string(), n, out, None, offs, 0)


def get_json_object(col: Column, path: str) -> Column:
    """Two passes of the row parser in json.hip. The size pass validates
    every row, matches the path and gives each row's output length, the
    matched value's span and a state (0 NULL, 1 value, 2 flagged); the write
    pass re-reads only the spans. Flagged rows, whose host rendering the
    device cannot reproduce, are compacted and answered by the CPU backend;
    every other row stays on the device."""
    from ..expr import json_path
    from . import cpu_backend

    return _json_path_single(
        col, json_path.parse(path),
        lambda flagged_rows: cpu_backend.get_json_object(flagged_rows, path))


def _all_null_strings(n: int) -> Column:
    return Column(DType.string(), n,
                  torch.empty(0, dtype=torch.uint8, device="cuda"),
                  torch.zeros(mask_nbytes(n), dtype=torch.uint8,
                              device="cuda"),
                  torch.zeros(n + 1, dtype=torch.int32, device="cuda"),
                  null_count=n)


def _json_path_single(col: Column, steps, ask_host) -> Column:
    """One path given as parsed steps; ask_host answers a host column of the
    flagged rows."""
    from ..expr import json_path

    n = col.size
    s = _stream()
    if n == 0:
        return _empty_col(DType.string())
    if steps is None:  # malformed path: NULL on every row
        return _all_null_strings(n)
    flat, names = json_path.encode(steps)
    steps_t = torch.tensor(flat or [0], dtype=torch.int32).cuda()
    names_t = torch.frombuffer(bytearray(names or b"\x00"),
                               dtype=torch.uint8).cuda()
    lens = torch.empty(n, dtype=torch.int64, device="cuda")
    ss = torch.empty(n, dtype=torch.int32, device="cuda")
    sl = torch.empty(n, dtype=torch.int32, device="cuda")
    state = torch.empty(n, dtype=torch.uint8, device="cuda")

    def run(mode, out_off=0, out_bytes=0):
        ext.json_path(col.offsets.data_ptr(), col.data.data_ptr(),
                      _ptr(col.validity), steps_t.data_ptr(),
                      names_t.data_ptr(), len(steps), out_off,
                      lens.data_ptr(), ss.data_ptr(), sl.data_ptr(),
                      state.data_ptr(), out_bytes, mode, n, s)

    def scan():
        scanned = torch.empty(n, dtype=torch.int64, device="cuda")
        scratch = torch.empty(ext.scan_scratch_elems(n), dtype=torch.int64,
                              device="cuda")
        ext.exclusive_scan_i64(lens.data_ptr(), scanned.data_ptr(),
                               scratch.data_ptr(), n, s)
        return scanned, scratch[-1]

    run(0)
    flagged = state == 2
    scanned, total_t = scan()
    # the one host read: output bytes and how many rows the host must answer
    total, nflag = torch.stack((total_t, flagged.sum())).tolist()
    host = None
    if nflag:
        fidx = torch.nonzero(flagged).flatten().to(torch.int32)
        host = ask_host(
            _gather_col(col, fidx, nflag, maybe_negative=False).cpu()).cuda()
        ho = host.offsets.to(torch.int64)
        hlens = ho[1:] - ho[:-1]
        lens[fidx.long()] = hlens
        scanned, total_t = scan()
        total = int(total_t.item())
    out_bytes = torch.empty(max(total, 1), dtype=torch.uint8,
                            device="cuda")[:total]
    if total:
        run(1, scanned.data_ptr(), out_bytes.data_ptr())
    if host is not None and host.data.numel():
        hdst = scanned[fidx.long()]
        ext.substr_copy(host.data.data_ptr(), host.offsets.data_ptr(),
                        hlens.data_ptr(), hdst.data_ptr(),
                        out_bytes.data_ptr(), nflag, s)
    offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), n, s)
    offs[n] = total
    v64 = state.to(torch.int64)
    if host is not None and host.validity is not None:
        hv = torch.empty(nflag, dtype=torch.uint8, device="cuda")
        ext.mask_expand(host.validity.data_ptr(), hv.data_ptr(), 0, nflag, s)
        v64[fidx.long()] = hv.to(torch.int64)
    mask = torch.empty(mask_nbytes(n), dtype=torch.uint8, device="cuda")
    ext.mask_from_nonzero(v64.data_ptr(), mask.data_ptr(), n, s)
    return Column(DType.string(), n, out_bytes, mask, offs, null_count=None)


def get_json_object_multi(col: Column, steps_list) -> List[Column]:
    """get_json_object for several paths over one column: one column per
    entry of steps_list (parsed steps; None, a malformed path, gives NULL on
    every row). Equal entries are computed once, and up to MAX_FUSED_PATHS
    distinct paths share one parse of each row."""
    from ..expr import json_path
    from . import cpu_backend

    n = col.size
    keys = [None if st is None else tuple(st) for st in steps_list]
    distinct = list(dict.fromkeys(k for k in keys if k is not None))
    done = {}
    if n == 0:
        return [_empty_col(DType.string()) for _ in keys]
    m = json_path.MAX_FUSED_PATHS
    for at in range(0, len(distinct), m):
        chunk = distinct[at:at + m]
        if len(chunk) == 1:
            steps = list(chunk[0])
            done[chunk[0]] = _json_path_single(
                col, steps, lambda rows, steps=steps:
                cpu_backend.get_json_object_steps(rows, steps))
        else:
            done.update(zip(chunk, _json_path_chunk(col, chunk)))
    return [_all_null_strings(n) if k is None else done[k] for k in keys]


def _json_path_chunk(col: Column, chunk) -> List[Column]:
    """2..MAX_FUSED_PATHS distinct paths in one size launch, one scan and one
    write launch. Every per-row array holds K * n entries, path-major, so
    path k owns [k * n, (k + 1) * n) and its column is a slice."""
    from ..expr import json_path
    from . import cpu_backend

    n = col.size
    s = _stream()
    K = len(chunk)
    # the native call launches nothing for a group size it has no kernel for
    assert 2 <= K <= json_path.MAX_FUSED_PATHS, K
    kn = K * n
    flat: List[int] = []
    names = bytearray()
    meta: List[int] = []       # step_off[K] then step_cnt[K]
    for steps in chunk:
        f, nm = json_path.encode(list(steps))
        for t in range(0, len(f), 3):
            if f[t] == json_path.KEY:
                f[t + 1] += len(names)
        meta.append(len(flat) // 3)
        flat.extend(f)
        names.extend(nm)
    meta.extend(len(steps) for steps in chunk)
    steps_t = torch.tensor(flat or [0], dtype=torch.int32).cuda()
    meta_t = torch.tensor(meta, dtype=torch.int32).cuda()
    names_t = torch.frombuffer(bytearray(names or b"\x00"),
                               dtype=torch.uint8).cuda()
    lens = torch.empty(kn, dtype=torch.int64, device="cuda")
    ss = torch.empty(kn, dtype=torch.int32, device="cuda")
    sl = torch.empty(kn, dtype=torch.int32, device="cuda")
    state = torch.empty(kn, dtype=torch.uint8, device="cuda")
    ext.json_path_multi(col.offsets.data_ptr(), col.data.data_ptr(),
                        _ptr(col.validity), steps_t.data_ptr(),
                        meta_t.data_ptr(), meta_t[K:].data_ptr(),
                        names_t.data_ptr(), K, lens.data_ptr(),
                        ss.data_ptr(), sl.data_ptr(), state.data_ptr(), n, s)

    def scan():
        scanned = torch.empty(kn, dtype=torch.int64, device="cuda")
        scratch = torch.empty(ext.scan_scratch_elems(kn), dtype=torch.int64,
                              device="cuda")
        ext.exclusive_scan_i64(lens.data_ptr(), scanned.data_ptr(),
                               scratch.data_ptr(), kn, s)
        # the total, then each path's first output position
        return scanned, torch.cat((scratch[-1:], scanned[::n]))

    flagged = state == 2
    scanned, ends_t = scan()
    # the one host read: output bytes, where each path's bytes begin, and how
    # many rows of each path the host must answer
    stats = torch.cat((ends_t, flagged.view(K, n).sum(dim=1))).tolist()
    total, base, nflags = stats[0], stats[1:K + 1], stats[K + 1:]
    hosts = {}
    for k, nflag in enumerate(nflags):
        if not nflag:
            continue
        fidx = torch.nonzero(flagged[k * n:(k + 1) * n]).flatten()
        host = cpu_backend.get_json_object_steps(
            _gather_col(col, fidx.to(torch.int32), nflag,
                        maybe_negative=False).cpu(), list(chunk[k])).cuda()
        ho = host.offsets.to(torch.int64)
        hlens = ho[1:] - ho[:-1]
        at = fidx + k * n
        lens[at] = hlens
        hosts[k] = (host, hlens, at)
    if hosts:
        scanned, ends_t = scan()
        ends = ends_t.tolist()
        total, base = ends[0], ends[1:]
    base.append(total)

    # One buffer for all paths, so that one write launch fills it, but each
    # column is a string column like any other: its data is the part of the
    # buffer that holds its own bytes (16-byte aligned starts, as a fresh
    # allocation's would be), its offsets start at 0 and end at data.numel().
    # Consumers such as concat_batches rely on both. Offsets are per path,
    # so int32 bounds a single path's bytes, never their sum.
    sizes = [base[k + 1] - base[k] for k in range(K)]
    starts, room = [], 0
    for size in sizes:
        starts.append(room)
        room += (size + 15) // 16 * 16
    place = torch.tensor([starts, base[:K], sizes], dtype=torch.int64).cuda()
    rel = scanned.view(K, n) - place[1].view(K, 1)   # within the path's bytes
    dst = (rel + place[0].view(K, 1)).view(-1)       # within the buffer
    out_bytes = torch.empty(max(room, 1), dtype=torch.uint8, device="cuda")
    if total:
        ext.json_path(0, col.data.data_ptr(), 0, 0, 0, 0, dst.data_ptr(),
                      lens.data_ptr(), ss.data_ptr(), sl.data_ptr(),
                      state.data_ptr(), out_bytes.data_ptr(), 1, kn, s)
    offs = torch.empty((K, n + 1), dtype=torch.int32, device="cuda")
    offs[:, :n] = rel
    offs[:, n] = place[2]
    v64 = state.to(torch.int64)
    for host, hlens, at in hosts.values():
        if host.data.numel():
            hdst = dst[at]
            ext.substr_copy(host.data.data_ptr(), host.offsets.data_ptr(),
                            hlens.data_ptr(), hdst.data_ptr(),
                            out_bytes.data_ptr(), hlens.numel(), s)
        if host.validity is not None:
            hv = torch.empty(at.numel(), dtype=torch.uint8, device="cuda")
            ext.mask_expand(host.validity.data_ptr(), hv.data_ptr(), 0,
                            at.numel(), s)
            v64[at] = hv.to(torch.int64)
    out = []
    for k in range(K):
        mask = torch.empty(mask_nbytes(n), dtype=torch.uint8, device="cuda")
        ext.mask_from_nonzero(v64[k * n:].data_ptr(), mask.data_ptr(), n, s)
        out.append(Column(DType.string(), n,
                          out_bytes[starts[k]:starts[k] + sizes[k]], mask,
                          offs[k], null_count=None))
    return out


def regexp_extract_all(col: Column, pattern: str, group: int) -> Column:
    """All matches' group text per row as LIST<STRING>."""
    n = col.size
    s = _stream()
    lt = DType.list_(DType.string())
    if n == 0:
        return Column.from_pylist([], lt).cuda()
    prog, prog_t, cls_t = _rx_prog_tensors(pattern)
    if group > prog.ngroups:
        raise ValueError(f"group {group} > {prog.ngroups}")
    counts = torch.empty(n, dtype=torch.int64, device="cuda")
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    ext.regex_extract_all(prog_t.data_ptr(), len(prog.ops),
                          cls_t.data_ptr(), col.offsets.data_ptr(),
                          col.data.data_ptr(), group, 0, counts.data_ptr(),
                          0, 0, 0, overflow.data_ptr(), n, s)
    if int(overflow.item()) > 0:
        from . import cpu_backend

        return cpu_backend.regexp_extract_all(col.cpu(), pattern,
                                              group).cuda()
    part_off, total = _exclusive_scan_i64(counts)
    ss = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")[:total]
    sl = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")[:total]
    if total:
        ext.regex_extract_all(prog_t.data_ptr(), len(prog.ops),
                              cls_t.data_ptr(), col.offsets.data_ptr(),
                              col.data.data_ptr(), group,
                              part_off.data_ptr(), counts.data_ptr(),
                              ss.data_ptr(), sl.data_ptr(), 1,
                              overflow.data_ptr(), n, s)
    scanned, nbytes = _exclusive_scan_i64(sl) if total else (sl, 0)
    out_bytes = torch.empty(max(nbytes, 1), dtype=torch.uint8,
                            device="cuda")[:nbytes]
    if nbytes:
        ext.substr_copy(col.data.data_ptr(), ss.data_ptr(), sl.data_ptr(),
                        scanned.data_ptr(), out_bytes.data_ptr(), total, s)
    coffs = torch.empty(total + 1, dtype=torch.int32, device="cuda")
    if total:
        ext.narrow_i64_i32(scanned.data_ptr(), coffs.data_ptr(), total, s)
    coffs[total] = nbytes
    child = Column(DType.string(), total, out_bytes, None, coffs, 0)
    loffs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(part_off.data_ptr(), loffs.data_ptr(), n, s)
    loffs[n] = total
    v = col.validity.clone() if col.validity is not None else None
    return Column(lt, n, torch.zeros(0, dtype=torch.uint8, device="cuda"),
                  v, loffs, col._null_count, child)


def regexp_replace(col: Column, pattern: str, replacement: str) -> Column:
    n = col.size
    s = _stream()
    if n == 0:
        return _empty_col(DType.string())
    prog, prog_t, cls_t = _rx_prog_tensors(pattern)
    ops_l, lit = _compile_replacement(replacement, prog.ngroups)
    flat = []
    for k, a, b in ops_l:
        flat.extend([k, a, b])
    repl_t = torch.tensor(flat or [0, 0, 0], dtype=torch.int32).cuda()
    lit_t = torch.frombuffer(bytearray(lit or b"\x00"),
                             dtype=torch.uint8).cuda()
    lens = torch.empty(n, dtype=torch.int64, device="cuda")
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")
    ext.regex_replace(prog_t.data_ptr(), len(prog.ops), cls_t.data_ptr(),
                      col.offsets.data_ptr(), col.data.data_ptr(),
                      repl_t.data_ptr(), len(ops_l), lit_t.data_ptr(),
                      0, lens.data_ptr(), 0, 0, overflow.data_ptr(), n, s)
    if int(overflow.item()) > 0:
        from . import cpu_backend

        return cpu_backend.regexp_replace(col.cpu(), pattern,
                                          replacement).cuda()
    scanned, total = _exclusive_scan_i64(lens)
    out_bytes = torch.empty(max(total, 1), dtype=torch.uint8,
                            device="cuda")[:total]
    if total:
        ext.regex_replace(prog_t.data_ptr(), len(prog.ops), cls_t.data_ptr(),
                          col.offsets.data_ptr(), col.data.data_ptr(),
                          repl_t.data_ptr(), len(ops_l), lit_t.data_ptr(),
                          scanned.data_ptr(), lens.data_ptr(),
                          out_bytes.data_ptr(), 1, overflow.data_ptr(), n, s)
    offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), n, s)
    offs[n] = total
    v = col.validity.clone() if col.validity is not None else None
    return Column(DType.string(), n, out_bytes, v, offs,
                  null_count=col._null_count)


def str_trim(col: Column, mode: str) -> Column:
    """trim/ltrim/rtrim (ascii space, Spark default)."""
    n = col.size
    s = _stream()
    if n == 0:
        return _empty_col(DType.string())
    m = {"both": 0, "leading": 1, "trailing": 2, "cast": 3}[mode]
    bstart = torch.empty(n, dtype=torch.int32, device="cuda")
    blen = torch.empty(n, dtype=torch.int64, device="cuda")
    ext.str_trim_ranges(m, col.offsets.data_ptr(), col.data.data_ptr(),
                        bstart.data_ptr(), blen.data_ptr(), n, s)
    return _strings_from_spans(col, bstart, blen, n, s)


def str_concat(a: Column, b: Column) -> Column:
    """concat(a, b): NULL if either side is NULL (Spark concat)."""
    n = a.size
    s = _stream()
    if n == 0:
        return _empty_col(DType.string())
    lens = torch.empty(n, dtype=torch.int64, device="cuda")
    ext.str_concat2(a.offsets.data_ptr(), a.data.data_ptr(),
                    b.offsets.data_ptr(), b.data.data_ptr(), 0,
                    lens.data_ptr(), 0, 0, n, s)
    scanned, total = _exclusive_scan_i64(lens)
    out_bytes = torch.empty(max(total, 1), dtype=torch.uint8,
                            device="cuda")[:total]
    if total:
        ext.str_concat2(a.offsets.data_ptr(), a.data.data_ptr(),
                        b.offsets.data_ptr(), b.data.data_ptr(),
                        scanned.data_ptr(), lens.data_ptr(),
                        out_bytes.data_ptr(), 1, n, s)
    offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), n, s)
    offs[n] = total
    v = _and_masks(a.validity, b.validity)
    return Column(DType.string(), n, out_bytes, v, offs,
                  null_count=None if v is not None else 0)


def str_split(col: Column, delimiter: str) -> Column:
    """Literal-delimiter split into LIST<STRING> (see StrSplit)."""
    n = col.size
    s = _stream()
    lt = DType.list_(DType.string())
    if n == 0:
        return Column.from_pylist([], lt).cuda()
    d = _pattern_tensor(delimiter)
    counts = torch.empty(n, dtype=torch.int64, device="cuda")
    ext.str_split_count(col.offsets.data_ptr(), col.data.data_ptr(),
                        d.data_ptr(), d.numel(), counts.data_ptr(), n, s)
    part_off, total = _exclusive_scan_i64(counts)
    ss = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")[:total]
    sl = torch.empty(max(total, 1), dtype=torch.int64, device="cuda")[:total]
    if total:
        ext.str_split_fill(col.offsets.data_ptr(), col.data.data_ptr(),
                           d.data_ptr(), d.numel(), part_off.data_ptr(),
                           counts.data_ptr(), ss.data_ptr(), sl.data_ptr(),
                           n, s)
    # child strings from (start, len) spans
    scanned, nbytes = _exclusive_scan_i64(sl) if total else (sl, 0)
    out_bytes = torch.empty(max(nbytes, 1), dtype=torch.uint8,
                            device="cuda")[:nbytes]
    if nbytes:
        ext.substr_copy(col.data.data_ptr(), ss.data_ptr(), sl.data_ptr(),
                        scanned.data_ptr(), out_bytes.data_ptr(), total, s)
    coffs = torch.empty(total + 1, dtype=torch.int32, device="cuda")
    if total:
        ext.narrow_i64_i32(scanned.data_ptr(), coffs.data_ptr(), total, s)
    coffs[total] = nbytes
    child = Column(DType.string(), total, out_bytes, None, coffs, 0)
    loffs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(part_off.data_ptr(), loffs.data_ptr(), n, s)
    loffs[n] = total
    v = col.validity.clone() if col.validity is not None else None
    return Column(lt, n, torch.zeros(0, dtype=torch.uint8, device="cuda"),
                  v, loffs, col._null_count, child)


def element_at(col: Column, index: int) -> Column:
    """Gather child elements at per-row offset +- index with bounds
    nullification (reuses the negative-index gather)."""
    n = col.size
    s = _stream()
    elem_dt = col.dtype.children[0]
    if n == 0:
        return _empty_col(elem_dt)
    starts = Column(DType.int32(), n, col.offsets[:n], None, null_count=0)
    ends = Column(DType.int32(), n, col.offsets[1:], None, null_count=0)
    if index > 0:
        idx = binary_op_scalar("add", starts, index - 1, DType.int32())
        ok = binary_op("lt", idx, ends, DType.bool_())
    else:
        idx = binary_op_scalar("add", ends, index, DType.int32())
        ok = binary_op("ge", idx, starts, DType.bool_())
    if col.validity is not None:
        # null list -> null element: fold into the gather index (-1 rows
        # nullify) so string elements need no typed if_else
        nn = unary_op("not", is_null(col), DType.bool_())
        ok = binary_op("and", ok, nn, DType.bool_())
    neg1 = Column.full(-1, DType.int32(), n, "cuda")
    srcm = if_else(ok, idx, neg1)
    return _gather_col(col.child, srcm.data, n, maybe_negative=True)


def array_contains(col: Column, value) -> Column:
    """Entry-level compare + per-segment any() via scatter amax."""
    n = col.size
    if n == 0:
        return _empty_col(DType.bool_())
    elem = col.child
    ne = elem.size
    hit = torch.zeros(n, dtype=torch.uint8, device="cuda")
    if ne:
        if elem.dtype.id is TypeId.STRING:
            sw = str_predicate("starts_with", elem, value)
            ln = unary_op("length", elem, DType.int32())
            lm = binary_op_scalar("eq", ln, len(value), DType.bool_())
            match = binary_op("and", sw, lm, DType.bool_())
        else:
            match = binary_op_scalar("eq", elem, value, DType.bool_())
        mt = match.data[:ne].bool()
        if elem.validity is not None:
            ev = torch.empty(ne, dtype=torch.uint8, device="cuda")
            ext.mask_expand(elem.validity.data_ptr(), ev.data_ptr(),
                            False, ne, _stream())
            mt &= ev.bool()
        offs = col.offsets.long()
        counts = offs[1:n + 1] - offs[:n]
        seg = torch.repeat_interleave(
            torch.arange(n, device="cuda", dtype=torch.int64), counts)
        if mt.any():
            hit.scatter_reduce_(0, seg[mt],
                                torch.ones(int(mt.sum()),
                                           dtype=torch.uint8,
                                           device="cuda"),
                                reduce="amax", include_self=True)
    v = col.validity.clone() if col.validity is not None else None
    return Column(DType.bool_(), n, hit, v, null_count=col._null_count)


def map_get(col: Column, key) -> Column:
    """element_at(map, key): entry-level key compare + per-segment
    last-match reduction (torch scatter_reduce amax over the entry iota),
    then a nullable gather of the value child."""
    n = col.size
    vdt = col.dtype.children[1]
    if n == 0:
        return _empty_col(vdt)
    entry = col.child
    kcol, vcol = entry.child
    ne = kcol.size
    if ne == 0:
        out = _gather_col(vcol, torch.full((n,), -1, dtype=torch.int32,
                                           device="cuda"), n,
                          maybe_negative=True)
        return out
    if kcol.dtype.id is TypeId.STRING:
        sw = str_predicate("starts_with", kcol, key)
        ln = unary_op("length", kcol, DType.int32())
        lm = binary_op_scalar("eq", ln, len(key), DType.bool_())
        match = binary_op("and", sw, lm, DType.bool_())
    else:
        match = binary_op_scalar("eq", kcol, key, DType.bool_())
    mt = match.data[:ne].bool()
    offs = col.offsets.long()
    counts = offs[1:n + 1] - offs[:n]
    seg = torch.repeat_interleave(
        torch.arange(n, device="cuda", dtype=torch.int64), counts)
    eidx = torch.arange(ne, device="cuda", dtype=torch.int64)
    res = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    if mt.any():
        res.scatter_reduce_(0, seg[mt], eidx[mt], reduce="amax",
                            include_self=True)
    if col.validity is not None:
        rv = torch.empty(n, dtype=torch.uint8, device="cuda")
        ext.mask_expand(col.validity.data_ptr(), rv.data_ptr(), False, n,
                        _stream())
        res = torch.where(rv.bool(), res,
                          torch.full_like(res, -1))
    return _gather_col(vcol, res.to(torch.int32), n, maybe_negative=True)


def make_map(kcols, vcols) -> Column:
    """create_map: interleave the per-pair key/value columns into entry
    children (block concat + permutation gather) with row-major offsets."""
    npairs = len(kcols)
    n = kcols[0].size
    dtype = DType.map_(kcols[0].dtype, vcols[0].dtype)
    perm_np = (np.arange(n * npairs, dtype=np.int32) % npairs) * n \
        + np.arange(n * npairs, dtype=np.int32) // npairs
    perm = torch.from_numpy(perm_np).cuda()
    def inter(cols):
        if len(cols) == 1:
            return cols[0]
        blk = concat_batches([ColumnBatch([c], n) for c in cols]).columns[0]
        return _gather_col(blk, perm, n * npairs, maybe_negative=False)
    kc = inter(kcols)
    vc = inter(vcols)
    entry = Column(dtype.entry_dtype, n * npairs,
                   torch.zeros(0, dtype=torch.uint8, device="cuda"),
                   None, None, 0, (kc, vc))
    offsets = torch.arange(0, (n + 1) * npairs, npairs,
                           dtype=torch.int32, device="cuda")
    return Column(dtype, n, torch.zeros(0, dtype=torch.uint8,
                                        device="cuda"),
                  None, offsets, 0, entry)


def array_size(col: Column) -> Column:
    n = col.size
    s = _stream()
    if n == 0:
        return _empty_col(DType.int32())
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    # sizes = offsets[i+1] - offsets[i] via the int32 sub kernel on views
    a = Column(DType.int32(), n, col.offsets[1:], None, null_count=0)
    b = Column(DType.int32(), n, col.offsets[:n], None, null_count=0)
    diff = _binary("sub", a, b, None, DType.int32())
    v = col.validity.clone() if col.validity is not None else None
    return Column(DType.int32(), n, diff.data, v,
                  null_count=col._null_count)


# ---------------------------------------------------------------------------
# lists: segmented sort / distinct / min / max (native/hipdf lists.hip)
# ---------------------------------------------------------------------------
_LT_STR = 7  # lists.hip element type id for a string child
_LIST_WAVE_MAX = 64  # longest list the sub-wave tier sorts


def _list_elem_args(elem: Column):
    """(type id, data ptr, element offsets ptr) of a LIST child."""
    if elem.dtype.id is TypeId.STRING:
        return _LT_STR, elem.data.data_ptr(), elem.offsets.data_ptr()
    return _ht(elem.dtype), elem.data.data_ptr(), 0


def _list_group_width(maxlen: int) -> int:
    w = 8
    while w < maxlen and w < _LIST_WAVE_MAX:
        w *= 2
    return w


def _list_bounds(col: Column):
    """(first offset, child rows covered, int32 lengths column, longest
    list) — one host sync each for the bounds and the maximum."""
    n = col.size
    off0, offn = (int(x) for x in col.offsets[0:n + 1:n].tolist())
    a = Column(DType.int32(), n, col.offsets[1:n + 1], None, null_count=0)
    b = Column(DType.int32(), n, col.offsets[:n], None, null_count=0)
    lens = _binary("sub", a, b, None, DType.int32())
    maxlen = int(reduce("max", lens) or 0)
    return off0, offn - off0, lens, maxlen


def _list_rebased_offsets(col: Column, off0: int) -> torch.Tensor:
    n = col.size
    if off0 == 0:
        return col.offsets[:n + 1].clone()
    oc = Column(DType.int32(), n + 1, col.offsets[:n + 1], None, null_count=0)
    return binary_op_scalar("sub", oc, off0, DType.int32()).data


def _list_with_child(col: Column, offsets: torch.Tensor,
                     child: Column) -> Column:
    v = col.validity.clone() if col.validity is not None else None
    return Column(col.dtype, col.size,
                  torch.zeros(0, dtype=torch.uint8, device="cuda"), v,
                  offsets, col._null_count, child)


def _list_sort_long(col: Column, lens: Column, cap: int, off0: int,
                    ascending: bool, nulls_first: bool,
                    perm: torch.Tensor) -> None:
    """Lists longer than the block tier's cap: the global radix sort over
    (row id, value) of only those rows, merged into `perm`. Index
    bookkeeping of this rare tier is host-driven torch arithmetic."""
    n = col.size
    rows = mask_to_sel(binary_op_scalar("gt", lens, cap, DType.bool_()), n)
    if rows.numel() == 0:
        return
    lr = rows.long()
    offs = col.offsets[:n + 1].long()
    starts = offs[lr]
    cnt = offs[lr + 1] - starts
    m = int(cnt.sum().item())
    seg = torch.repeat_interleave(
        torch.arange(lr.numel(), device="cuda", dtype=torch.int64), cnt)
    base = torch.cumsum(cnt, 0) - cnt
    eidx = (torch.arange(m, device="cuda", dtype=torch.int64)
            - base[seg] + starts[seg]).to(torch.int32)
    vals = _gather_col(col.child, eidx, m, maybe_negative=False)
    segc = Column(DType.int32(), m, seg.to(torch.int32), None, null_count=0)
    order = sort_order(ColumnBatch([segc, vals], m), [0, 1],
                       [False, not ascending], [False, not nulls_first])
    perm[eidx.long() - off0] = eidx[order.data.long()]


def _list_sort_perm(col: Column, ascending: bool, nulls_first: bool):
    """Permutation of global child indices that sorts every list in place:
    (perm or None when no elements, first offset, elements covered)."""
    n = col.size
    s = _stream()
    elem = col.child
    off0, total, lens, maxlen = _list_bounds(col)
    if total == 0:
        return None, off0, 0
    t, dp, eo = _list_elem_args(elem)
    perm = torch.empty(total, dtype=torch.int32, device="cuda")
    ext.list_sort_wave(t, dp, eo, _ptr(elem.validity),
                       col.offsets.data_ptr(), _list_group_width(maxlen),
                       nulls_first, not ascending, perm.data_ptr(), n, s)
    if maxlen > _LIST_WAVE_MAX:
        cap = ext.list_block_cap()
        mid = binary_op(
            "and", binary_op_scalar("gt", lens, _LIST_WAVE_MAX, DType.bool_()),
            binary_op_scalar("le", lens, cap, DType.bool_()), DType.bool_())
        rows = mask_to_sel(mid, n)
        if rows.numel():
            ext.list_sort_block(t, dp, eo, _ptr(elem.validity),
                                col.offsets.data_ptr(), rows.data_ptr(),
                                rows.numel(), nulls_first, not ascending,
                                perm.data_ptr(), s)
        if maxlen > cap:
            _list_sort_long(col, lens, cap, off0, ascending, nulls_first,
                            perm)
    return perm, off0, total


def sort_array(col: Column, ascending: bool = True,
               nulls_first: bool = True) -> Column:
    """Segmented stable sort of every list; the permutation goes through
    the ordinary gather so validity and string bytes follow."""
    n = col.size
    if n == 0:
        return Column.from_pylist([], col.dtype).cuda()
    perm, off0, total = _list_sort_perm(col, ascending, nulls_first)
    child = _gather_col(col.child, perm, total, maybe_negative=False) \
        if total else _empty_col(col.child.dtype)
    return _list_with_child(col, _list_rebased_offsets(col, off0), child)


def array_distinct(col: Column) -> Column:
    """Ascending segmented sort -> duplicate flags against the sorted
    predecessor -> scan -> compaction in original order (KEEP_FIRST)."""
    n = col.size
    s = _stream()
    if n == 0:
        return Column.from_pylist([], col.dtype).cuda()
    elem = col.child
    perm, off0, total = _list_sort_perm(col, True, True)
    if total == 0:
        return _list_with_child(col, _list_rebased_offsets(col, off0),
                                _empty_col(elem.dtype))
    keep = _list_distinct_flags(col, perm, total)
    new_offs, child = _list_compact(col, keep, off0, total)
    return _list_with_child(col, new_offs, child)


def _list_distinct_flags(col: Column, perm: torch.Tensor,
                         total: int) -> torch.Tensor:
    """uint8[total], 1 at the first occurrence of each value of its list;
    `perm` is the ascending nulls-first `_list_sort_perm` (total > 0)."""
    elem = col.child
    t, dp, eo = _list_elem_args(elem)
    keep = torch.empty(total, dtype=torch.uint8, device="cuda")
    ext.list_distinct_flags(t, dp, eo, _ptr(elem.validity),
                            col.offsets.data_ptr(), col.size,
                            perm.data_ptr(), keep.data_ptr(), total,
                            _stream())
    return keep


def _list_keep_scan(keep: Optional[torch.Tensor], total: int):
    """(exclusive scan of the uint8 keep flags as int64[total + 1], kept
    count): kept-before counts at every element, one extra slot for the
    total."""
    keep64 = torch.zeros(total + 1, dtype=torch.int64, device="cuda")
    if total:
        ext.cast(0, 4, keep.data_ptr(), keep64.data_ptr(), total, _stream())
    return _exclusive_scan_i64(keep64)


def _list_compact(col: Column, keep: torch.Tensor, off0: int, total: int):
    """Drop the elements whose uint8 keep flag (one per element from
    `off0`, total > 0) is 0, order kept: (new int32 offsets, new child)."""
    n = col.size
    s = _stream()
    scanned, nkept = _list_keep_scan(keep, total)
    rebased = _list_rebased_offsets(col, off0)
    offs64 = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ext.gather_fixed(8, scanned.data_ptr(), rebased.data_ptr(),
                     offs64.data_ptr(), n + 1, s)
    new_offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(offs64.data_ptr(), new_offs.data_ptr(), n + 1, s)
    sel = mask_to_sel(Column(DType.bool_(), total, keep, None, null_count=0),
                      total)
    if off0:
        sel = binary_op_scalar(
            "add", Column(DType.int32(), nkept, sel, None, null_count=0),
            off0, DType.int32()).data
    child = _gather_col(col.child, sel, nkept, maybe_negative=False)
    return new_offs, child


# two-list set operations: a is probed against b's sorted rows

def _list_pair_check(a: Column, b: Column) -> None:
    if a.dtype.id is not TypeId.LIST or a.dtype != b.dtype:
        raise TypeError("array set operations need two arrays of one "
                        f"element type, got {a.dtype} and {b.dtype}")
    if a.size != b.size:
        raise ValueError(f"array operands of {a.size} and {b.size} rows")


def _list_pair_validity(a: Column, b: Column):
    v = _and_masks(a.validity, b.validity)
    return v, (None if v is not None else 0)


def _list_member_flags(a: Column, atotal: int, b: Column,
                       bperm: Optional[torch.Tensor]) -> torch.Tensor:
    """uint8[atotal], 1 where the element of `a` has an equal element in
    the same row of `b`; `bperm` is b's ascending nulls-first
    `_list_sort_perm` (None when b has no elements)."""
    t, adp, aeo = _list_elem_args(a.child)
    _, bdp, beo = _list_elem_args(b.child)
    member = torch.empty(atotal, dtype=torch.uint8, device="cuda")
    ext.list_member_flags(t, adp, aeo, _ptr(a.child.validity),
                          a.offsets.data_ptr(), bdp, beo,
                          _ptr(b.child.validity), b.offsets.data_ptr(),
                          _ptr(bperm), a.size, member.data_ptr(), atotal,
                          _stream())
    return member


def _flag_col(flags: torch.Tensor) -> Column:
    return Column(DType.bool_(), flags.numel(), flags, None, null_count=0)


def _array_filter_by_member(a: Column, b: Column, negate: bool) -> Column:
    """distinct(a) AND member (array_intersect), or AND NOT member
    (array_except), compacted in a's order."""
    _list_pair_check(a, b)
    n = a.size
    if n == 0:
        return Column.from_pylist([], a.dtype).cuda()
    v, nc = _list_pair_validity(a, b)
    aperm, aoff0, atotal = _list_sort_perm(a, True, True)
    if atotal == 0:
        new_offs, child = _list_rebased_offsets(a, aoff0), \
            _empty_col(a.child.dtype)
    else:
        bperm, _, _ = _list_sort_perm(b, True, True)
        member = _flag_col(_list_member_flags(a, atotal, b, bperm))
        if negate:
            member = unary_op("not", member, DType.bool_())
        keep = binary_op("and", _flag_col(_list_distinct_flags(a, aperm,
                                                               atotal)),
                         member, DType.bool_()).data
        new_offs, child = _list_compact(a, keep, aoff0, atotal)
    return Column(a.dtype, n, torch.zeros(0, dtype=torch.uint8, device="cuda"),
                  v, new_offs, nc, child)


def array_intersect(a: Column, b: Column) -> Column:
    """First occurrences of a's elements that occur in b's row, a's order
    and bit patterns."""
    return _array_filter_by_member(a, b, False)


def array_except(a: Column, b: Column) -> Column:
    """First occurrences of a's elements that do not occur in b's row."""
    return _array_filter_by_member(a, b, True)


def array_union(a: Column, b: Column) -> Column:
    """distinct(a) followed by distinct(b) AND NOT member-of-a, per row:
    one gather map over concat(a.child, b.child) (list_union_map)."""
    _list_pair_check(a, b)
    n = a.size
    s = _stream()
    if n == 0:
        return Column.from_pylist([], a.dtype).cuda()
    v, nc = _list_pair_validity(a, b)
    aperm, _, atotal = _list_sort_perm(a, True, True)
    bperm, _, btotal = _list_sort_perm(b, True, True)
    akeep = _list_distinct_flags(a, aperm, atotal) if atotal else None
    bkeep = None
    if btotal:
        bkeep = _list_distinct_flags(b, bperm, btotal)
        if atotal:
            fresh = unary_op("not", _flag_col(
                _list_member_flags(b, btotal, a, aperm)), DType.bool_())
            bkeep = binary_op("and", _flag_col(bkeep), fresh,
                              DType.bool_()).data
    ascan, na = _list_keep_scan(akeep, atotal)
    bscan, nb = _list_keep_scan(bkeep, btotal)
    nkept = na + nb
    if nkept > 2 ** 31 - 1:
        raise OverflowError("array_union result exceeds int32 offsets")
    new_offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    idx = torch.empty(max(nkept, 1), dtype=torch.int32, device="cuda")[:nkept]
    ext.list_union_map(ascan.data_ptr(), a.offsets.data_ptr(), atotal,
                       bscan.data_ptr(), b.offsets.data_ptr(), btotal, n,
                       a.child.size, new_offs.data_ptr(), idx.data_ptr(), s)
    if nkept:
        both = concat_batches([ColumnBatch([a.child], a.child.size),
                               ColumnBatch([b.child], b.child.size)])
        child = _gather_col(both.columns[0], idx, nkept, maybe_negative=False)
    else:
        child = _empty_col(a.child.dtype)
    return Column(a.dtype, n, torch.zeros(0, dtype=torch.uint8, device="cuda"),
                  v, new_offs, nc, child)


def arrays_overlap(a: Column, b: Column) -> Column:
    """True when a non-null element is shared, else NULL when both rows are
    non-empty and either holds a null, else false (list_overlap)."""
    _list_pair_check(a, b)
    n = a.size
    if n == 0:
        return _empty_col(DType.bool_())
    aoff0, atotal, _, amax = _list_bounds(a)
    bperm, _, btotal = _list_sort_perm(b, True, True)
    member = _list_member_flags(a, atotal, b, bperm) if atotal else None
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    ov = _alloc_mask(n)
    ext.list_overlap(_ptr(member), a.offsets.data_ptr(),
                     _ptr(a.child.validity), _ptr(a.validity),
                     b.offsets.data_ptr(), _ptr(b.child.validity),
                     _ptr(b.validity), _ptr(bperm), _list_group_width(amax),
                     out.data_ptr(), ov.data_ptr(), n, _stream())
    return Column(DType.bool_(), n, out, ov, null_count=None)


# higher-order functions: the lambda body runs as ordinary column kernels
# over the flattened child; these map elements to rows and fold a predicate
# column (one BOOL per element from offsets[0]) back into rows

def list_span(col: Column):
    """(first offset, child rows covered) — the one host read."""
    n = col.size
    if n == 0:
        return 0, 0
    off0, offn = (int(x) for x in col.offsets[0:n + 1:n].tolist())
    return off0, offn - off0


def list_element_rows(col: Column, with_pos: bool = True, span=None):
    """(rowid, pos): int32 columns with one row per element from
    offsets[0], the owning row and the 0-based place in it (pos is None
    unless asked for)."""
    off0, total = span or list_span(col)
    rowid = torch.empty(max(total, 1), dtype=torch.int32,
                        device="cuda")[:total]
    pos = torch.empty_like(rowid) if with_pos else None
    ext.list_elem_rows(col.offsets.data_ptr(), col.size, rowid.data_ptr(),
                       _ptr(pos), total, _stream())
    return (Column(DType.int32(), total, rowid, None, null_count=0),
            None if pos is None else
            Column(DType.int32(), total, pos, None, null_count=0))


def _check_pred(pred: Column, total: int) -> None:
    if pred.dtype.id is not TypeId.BOOL or pred.size != total:
        raise ValueError(f"predicate of {pred.size} {pred.dtype} rows for "
                         f"{total} array elements")


def array_filter(col: Column, pred: Column, span=None) -> Column:
    """Keep the elements whose predicate is true and not null, order kept;
    the compaction is array_distinct's."""
    n = col.size
    if n == 0:
        return Column.from_pylist([], col.dtype).cuda()
    off0, total = span or list_span(col)
    _check_pred(pred, total)
    if total == 0:
        return _list_with_child(col, _list_rebased_offsets(col, off0),
                                _empty_col(col.child.dtype))
    keep = pred.data[:total]
    if pred.validity is not None:
        ok = torch.empty(total, dtype=torch.uint8, device="cuda")
        ext.mask_expand(pred.validity.data_ptr(), ok.data_ptr(), False,
                        total, _stream())
        keep = binary_op("and", _flag_col(keep), _flag_col(ok),
                         DType.bool_()).data
    new_offs, child = _list_compact(col, keep, off0, total)
    return _list_with_child(col, new_offs, child)


def _list_bool_reduce(col: Column, pred: Column, mode: int,
                      span) -> Column:
    n = col.size
    if n == 0:
        return _empty_col(DType.bool_())
    _, total = span or list_span(col)
    _check_pred(pred, total)
    if total == 0:  # every row is empty or null
        v = col.validity.clone() if col.validity is not None else None
        return Column(DType.bool_(), n,
                      torch.full((n,), mode, dtype=torch.uint8,
                                 device="cuda"), v, null_count=col._null_count)
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    ov = _alloc_mask(n)
    # lanes per row from the mean length: no maximum-length sync, and the
    # stride covers the rows that are longer
    ext.list_bool_reduce(pred.data.data_ptr(), _ptr(pred.validity),
                         col.offsets.data_ptr(), _ptr(col.validity),
                         _list_group_width(-(-total // n)), mode,
                         out.data_ptr(), ov.data_ptr(), n, _stream())
    return Column(DType.bool_(), n, out, ov, null_count=None)


def array_exists(col: Column, pred: Column, span=None) -> Column:
    """True when a predicate of the row is true, else NULL when one is
    null, else false (list_bool_reduce)."""
    return _list_bool_reduce(col, pred, 0, span)


def array_forall(col: Column, pred: Column, span=None) -> Column:
    """False when a predicate of the row is false, else NULL when one is
    null, else true."""
    return _list_bool_reduce(col, pred, 1, span)


# search, slice, repeat: a per-row scalar operand next to the array

def _list_needle_check(fn: str, col: Column, needle: Column) -> None:
    if col.dtype.id is not TypeId.LIST or needle.dtype != col.dtype.children[0]:
        raise TypeError(f"{fn} needs an array and a value of its element "
                        f"type, got {col.dtype} and {needle.dtype}")
    if needle.size != col.size:
        raise ValueError(f"{fn}: {col.size} arrays and {needle.size} values")


def _list_find(col: Column, needle: Column, total: int, want_match: bool,
               want_first: bool):
    """(match uint8[total] or None, first int64[n] or None, validity of
    row AND needle) from one list_find launch; n > 0 and total > 0."""
    n = col.size
    t, dp, eo = _list_elem_args(col.child)
    _, ndp, neo = _list_elem_args(needle)
    match = torch.empty(total, dtype=torch.uint8, device="cuda") \
        if want_match else None
    first = torch.empty(n, dtype=torch.int64, device="cuda") \
        if want_first else None
    ov = _alloc_mask(n)
    # lanes per row from the mean length, as list_bool_reduce
    ext.list_find(t, dp, eo, _ptr(col.child.validity), col.offsets.data_ptr(),
                  _ptr(col.validity), ndp, neo, _ptr(needle.validity),
                  _list_group_width(-(-total // n)), _ptr(match), _ptr(first),
                  ov.data_ptr(), n, _stream())
    return match, first, ov


def array_position(col: Column, needle: Column) -> Column:
    """1-based place of the first element equal to the row's needle, 0 for
    none; NULL when the row or the needle is (list_find)."""
    _list_needle_check("array_position", col, needle)
    n = col.size
    if n == 0:
        return _empty_col(DType.int64())
    _, total = list_span(col)
    if total == 0:  # every row is empty or null
        v = _and_masks(col.validity, needle.validity)
        return Column(DType.int64(), n,
                      torch.zeros(n, dtype=torch.int64, device="cuda"), v,
                      null_count=None if v is not None else 0)
    _, first, ov = _list_find(col, needle, total, False, True)
    return Column(DType.int64(), n, first, ov, null_count=None)


def array_remove(col: Column, needle: Column) -> Column:
    """The array without the elements equal to the row's needle, order and
    null elements kept; NULL when the row or the needle is. list_find's
    match flags, negated, go through array_distinct's compaction."""
    _list_needle_check("array_remove", col, needle)
    n = col.size
    if n == 0:
        return Column.from_pylist([], col.dtype).cuda()
    off0, total = list_span(col)
    empty = torch.zeros(0, dtype=torch.uint8, device="cuda")
    if total == 0:
        v = _and_masks(col.validity, needle.validity)
        return Column(col.dtype, n, empty, v, _list_rebased_offsets(col, off0),
                      None if v is not None else 0,
                      _empty_col(col.child.dtype))
    match, _, ov = _list_find(col, needle, total, True, False)
    keep = unary_op("not", _flag_col(match), DType.bool_()).data
    new_offs, child = _list_compact(col, keep, off0, total)
    return Column(col.dtype, n, empty, ov, new_offs, None, child)


def _int32_operand(fn: str, what: str, c: Column, n: int) -> Column:
    if c.dtype.id is not TypeId.INT32:
        raise TypeError(f"{fn}: {what} must be INT32, got {c.dtype}")
    if c.size != n:
        raise ValueError(f"{fn}: {n} rows and {c.size} {what} values")
    return c


def array_slice(col: Column, start: Column, length: Column) -> Column:
    """slice(array, start, length): list_slice_ranges turns the three
    operands into a first child index and a length per row, the lengths
    scan into the new offsets, list_slice_map writes the gather map."""
    if col.dtype.id is not TypeId.LIST:
        raise TypeError(f"slice needs an array input, got {col.dtype}")
    n = col.size
    s = _stream()
    _int32_operand("slice", "start", start, n)
    _int32_operand("slice", "length", length, n)
    if n == 0:
        return Column.from_pylist([], col.dtype).cuda()
    src_start = torch.empty(n, dtype=torch.int32, device="cuda")
    out_len = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ov = _alloc_mask(n)
    err = torch.zeros(2, dtype=torch.int64, device="cuda")
    ext.list_slice_ranges(col.offsets.data_ptr(), _ptr(col.validity),
                          start.data.data_ptr(), _ptr(start.validity),
                          length.data.data_ptr(), _ptr(length.validity),
                          src_start.data_ptr(), out_len.data_ptr(),
                          ov.data_ptr(), err.data_ptr(), n, s)
    # the error record comes back with the scan total, one blocking read
    scanned, total, (bad_start, bad_len) = _exclusive_scan_i64(out_len, err)
    if bad_start:
        raise ValueError(SLICE_START_ERROR)
    if bad_len:
        raise ValueError(SLICE_LENGTH_ERROR)
    new_offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(scanned.data_ptr(), new_offs.data_ptr(), n + 1, s)
    if total:
        idx = torch.empty(total, dtype=torch.int32, device="cuda")
        ext.list_slice_map(new_offs.data_ptr(), src_start.data_ptr(), n,
                           idx.data_ptr(), total, s)
        child = _gather_col(col.child, idx, total, maybe_negative=False)
    else:
        child = _empty_col(col.child.dtype)
    return Column(col.dtype, n, torch.zeros(0, dtype=torch.uint8,
                                            device="cuda"),
                  ov, new_offs, None, child)


def array_repeat(elem: Column, count: Column) -> Column:
    """count copies of the row's element (a null element gives nulls), no
    copies for count <= 0, NULL for a null count. The lengths scan into
    the offsets; the element-to-row map over them is the gather map."""
    n = elem.size
    s = _stream()
    _int32_operand("array_repeat", "count", count, n)
    dtype = DType.list_(elem.dtype)
    if n == 0:
        return Column.from_pylist([], dtype).cuda()
    lens = binary_op_scalar("max", count, 0, DType.int32())
    if count.validity is not None:
        present = unary_op("not", is_null(count), DType.bool_())
        lens = if_else(present, lens, Column.full(0, DType.int32(), n, "cuda"))
    lens64 = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    ext.cast(_ht(DType.int32()), _ht(DType.int64()), lens.data.data_ptr(),
             lens64.data_ptr(), n, s)
    scanned, total = _exclusive_scan_i64(lens64)
    if total > 2 ** 31 - 1:
        raise OverflowError("array_repeat result exceeds int32 offsets")
    new_offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(scanned.data_ptr(), new_offs.data_ptr(), n + 1, s)
    if total:
        rowid = torch.empty(total, dtype=torch.int32, device="cuda")
        ext.list_elem_rows(new_offs.data_ptr(), n, rowid.data_ptr(), 0, total,
                           s)
        child = _gather_col(elem, rowid, total, maybe_negative=False)
    else:
        child = _empty_col(elem.dtype)
    v = count.validity.clone() if count.validity is not None else None
    return Column(dtype, n, torch.zeros(0, dtype=torch.uint8, device="cuda"),
                  v, new_offs, count._null_count, child)


# builders: array(), concat, flatten, sequence, array_join

_LIST_MAX_OPERANDS = 8  # HIPDF_LIST_MAX_OPERANDS: operands of one launch
_NO_DATA = dict(dtype=torch.uint8, device="cuda")


def _list_operands(ptrs, valids) -> torch.Tensor:
    """HipdfListOperands in host memory for up to 8 operands; the entry
    point reads it during the call and hands it to the kernel by value."""
    pad = [0] * (_LIST_MAX_OPERANDS - len(ptrs))
    return torch.frombuffer(
        bytearray(struct.pack("<16q", *ptrs, *pad, *valids, *pad)),
        dtype=torch.uint8)


def _no_nested(fn: str, et: DType) -> None:
    if et.is_nested:
        raise NotImplementedError(f"{fn} over nested elements runs on the "
                                  "CPU")


def _concat_cols(cols) -> Column:
    if len(cols) == 1:
        return cols[0]
    return concat_batches([ColumnBatch([c], c.size) for c in cols]).columns[0]


def create_array(cols) -> Column:
    """array(c1, ..., ck). Fixed-width operands (<= 64 bit) go through
    list_interleave, 8 per launch; strings and decimal128 through one
    gather over the concatenated operands (list_interleave_map)."""
    _same_type_operands("array", cols, False)
    k, n, et = len(cols), cols[0].size, cols[0].dtype
    _no_nested("array", et)
    dtype = DType.list_(et)
    s = _stream()
    if n == 0:
        return Column.from_pylist([], dtype).cuda()
    total = n * k
    if total > 2 ** 31 - 1:
        raise OverflowError("array result exceeds int32 offsets")
    new_offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    if et.id in (TypeId.STRING, TypeId.DECIMAL128):
        idx = torch.empty(total, dtype=torch.int32, device="cuda")
        ext.list_interleave_map(k, idx.data_ptr(), new_offs.data_ptr(), n, s)
        child = _gather_col(_concat_cols(cols), idx, total,
                            maybe_negative=False)
    else:
        out = _alloc(total, et)
        shared = k > _LIST_MAX_OPERANDS  # launches share validity words
        ov = None
        if any(c.validity is not None for c in cols):
            ov = torch.zeros(mask_nbytes(total), **_NO_DATA) if shared \
                else _alloc_mask(total)
        for j0 in range(0, k, _LIST_MAX_OPERANDS):
            part = cols[j0:j0 + _LIST_MAX_OPERANDS]
            ops_ = _list_operands([c.data.data_ptr() for c in part],
                                  [_ptr(c.validity) for c in part])
            ext.list_interleave(et.itemsize, ops_.data_ptr(), k, j0,
                                len(part), int(shared), out.data_ptr(),
                                _ptr(ov), new_offs.data_ptr() if j0 == 0
                                else 0, n, s)
        child = Column(et, total, out, ov,
                       null_count=None if ov is not None else 0)
    return Column(dtype, n, torch.zeros(0, **_NO_DATA), None, new_offs, 0,
                  child)


def array_concat(cols) -> Column:
    """concat(a1, ..., ak): list_concat_lens sums the rows' lengths (8
    operands per launch), they scan into the offsets, list_concat_map
    writes one gather map over the concatenated children."""
    _same_type_operands("concat", cols, True)
    k, n, dtype = len(cols), cols[0].size, cols[0].dtype
    _no_nested("concat", dtype.children[0])
    s = _stream()
    if n == 0:
        return Column.from_pylist([], dtype).cuda()
    bases = [0]
    for c in cols:
        bases.append(bases[-1] + c.child.size)
    if bases[-1] > 2 ** 31 - 1:
        raise OverflowError("concat operands exceed an int32 gather map")
    out_len = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ov = _alloc_mask(n)
    launches = []  # (operand block, operand count, base rows, prefix)
    for j0 in range(0, k, _LIST_MAX_OPERANDS):
        part = cols[j0:j0 + _LIST_MAX_OPERANDS]
        ops_ = _list_operands([c.offsets.data_ptr() for c in part],
                              [_ptr(c.validity) for c in part])
        prefix = torch.empty(n, dtype=torch.int32, device="cuda") \
            if j0 else None
        ext.list_concat_lens(ops_.data_ptr(), len(part), int(j0 == 0),
                             int(j0 + _LIST_MAX_OPERANDS >= k),
                             out_len.data_ptr(), _ptr(prefix), ov.data_ptr(),
                             n, s)
        launches.append((ops_, len(part), bases[j0:j0 + len(part)], prefix))
    scanned, total = _exclusive_scan_i64(out_len)
    if total > 2 ** 31 - 1:
        raise OverflowError("concat result exceeds int32 offsets")
    new_offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(scanned.data_ptr(), new_offs.data_ptr(), n + 1, s)
    if total:
        idx = torch.empty(total, dtype=torch.int32, device="cuda")
        for ops_, kk, base, prefix in launches:
            cbase = torch.tensor(base, dtype=torch.int64)
            ext.list_concat_map(ops_.data_ptr(), cbase.data_ptr(), kk,
                                new_offs.data_ptr(), _ptr(prefix), n,
                                idx.data_ptr(), total, s)
        child = _gather_col(_concat_cols([c.child for c in cols]), idx, total,
                            maybe_negative=False)
    else:
        child = _empty_col(dtype.children[0])
    return Column(dtype, n, torch.zeros(0, **_NO_DATA), ov, new_offs, None,
                  child)


def _rows_view(c: Column, first: int, end: int) -> Column:
    """Rows [first, end) of a flat column: a view where the buffers allow
    one (validity words must start on a word), else a gather."""
    m = end - first
    if m == 0:
        return _empty_col(c.dtype)
    if first == 0 and end == c.size:
        return c
    plain = not isinstance(c, DictColumn) and c.dtype.id is not TypeId.STRUCT
    if plain and (c.validity is None or first % 64 == 0):
        v = None if c.validity is None else c.validity[first // 8:]
        nc = None if v is not None else 0
        if c.dtype.id is not TypeId.STRING:
            w = 2 if c.dtype.id is TypeId.DECIMAL128 else 1
            return Column(c.dtype, m, c.data[first * w:end * w], v,
                          null_count=nc)
        if first == 0:  # string offsets stay absolute, so only a prefix
            return Column(c.dtype, m, c.data, v, c.offsets[:m + 1], nc)
    idx = torch.empty(m, dtype=torch.int32, device="cuda")
    ext.iota_i32(idx.data_ptr(), m, _stream())
    if first:
        idx = binary_op_scalar(
            "add", Column(DType.int32(), m, idx, None, null_count=0), first,
            DType.int32()).data
    return _gather_col(c, idx, m, maybe_negative=False)


def array_flatten(col: Column) -> Column:
    """flatten(LIST<LIST<T>>): list_flatten composes the two offset arrays
    and folds the inner validity into the rows'; the innermost child is
    the result's child, cut to the rows' span."""
    if col.dtype.id is not TypeId.LIST or \
            col.dtype.children[0].id is not TypeId.LIST:
        raise TypeError(f"flatten needs an array of arrays, got {col.dtype}")
    dtype = col.dtype.children[0]
    _no_nested("flatten", dtype.children[0])
    n = col.size
    if n == 0:
        return Column.from_pylist([], dtype).cuda()
    inner = col.child
    new_offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ov = _alloc_mask(n)
    span = torch.empty(2, dtype=torch.int64, device="cuda")
    # 8 lanes per row: the inner arrays of a row are few
    ext.list_flatten(col.offsets.data_ptr(), _ptr(col.validity),
                     inner.offsets.data_ptr(), _ptr(inner.validity), 8,
                     new_offs.data_ptr(), ov.data_ptr(), span.data_ptr(), n,
                     _stream())
    first, end = (int(x) for x in span.tolist())  # the one host read
    return Column(dtype, n, torch.zeros(0, **_NO_DATA), ov, new_offs, None,
                  _rows_view(inner.child, first, end))


def sequence(start: Column, stop: Column,
             step: Optional[Column] = None) -> Column:
    """sequence(start, stop[, step]): sequence_ranges gives the lengths,
    the validity and the first illegal row with its values, which comes
    back with the scan total; sequence_fill writes the elements."""
    _sequence_operands(start, stop, step)
    n = start.size
    s = _stream()
    dtype = DType.list_(start.dtype)
    if n == 0:
        return Column.from_pylist([], dtype).cuda()
    t = _ht(start.dtype)
    out_len = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ov = _alloc_mask(n)
    err = torch.tensor([2 ** 63 - 1, 0, 0, 0], dtype=torch.int64).cuda()
    step_ptr = step.data.data_ptr() if step is not None else 0
    ext.sequence_ranges(t, start.data.data_ptr(), _ptr(start.validity),
                        stop.data.data_ptr(), _ptr(stop.validity), step_ptr,
                        _ptr(step.validity) if step is not None else 0,
                        out_len.data_ptr(), ov.data_ptr(), err.data_ptr(), n,
                        s)
    scanned, total, (bad, a, b, st) = _exclusive_scan_i64(out_len, err)
    if bad < n:
        raise ValueError(SEQUENCE_ERROR.format(a, b, st))
    if total > 2 ** 31 - 1:
        raise OverflowError(SEQUENCE_OVERFLOW)
    new_offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(scanned.data_ptr(), new_offs.data_ptr(), n + 1, s)
    out = _alloc(total, start.dtype)
    ext.sequence_fill(t, new_offs.data_ptr(), start.data.data_ptr(),
                      stop.data.data_ptr(), step_ptr, n, out.data_ptr(),
                      total, s)
    child = Column(start.dtype, total, out, None, null_count=0)
    return Column(dtype, n, torch.zeros(0, **_NO_DATA), ov, new_offs, None,
                  child)


def array_join(col: Column, delimiter: str,
               null_replacement: Optional[str] = None) -> Column:
    """array_join: array_join_sizes gives every element's bytes with its
    delimiter, their scan places the elements, array_join_rows turns it
    into row lengths, whose scan gives the string offsets, and
    array_join_write copies element-parallel."""
    if col.dtype.id is not TypeId.LIST or \
            col.dtype.children[0].id is not TypeId.STRING:
        raise TypeError(f"array_join needs an array of strings, got "
                        f"{col.dtype}")
    n = col.size
    s = _stream()
    if n == 0:
        return _empty_col(DType.string())
    v = col.validity.clone() if col.validity is not None else None
    _, total = list_span(col)
    if total == 0:  # every row is empty or null
        return Column(DType.string(), n, torch.zeros(0, **_NO_DATA), v,
                      torch.zeros(n + 1, dtype=torch.int32, device="cuda"),
                      col._null_count)
    d = _pattern_tensor(delimiter)
    has_repl = null_replacement is not None
    r = _pattern_tensor(null_replacement if has_repl else "")
    dlen, rlen = d.numel(), (r.numel() if has_repl else -1)
    ch = col.child
    contrib = torch.empty(total + 1, dtype=torch.int64, device="cuda")
    ext.array_join_sizes(col.offsets.data_ptr(), _ptr(col.validity),
                         ch.offsets.data_ptr(), _ptr(ch.validity), dlen, rlen,
                         n, contrib.data_ptr(), total, s)
    placed, _ = _exclusive_scan_i64(contrib)
    out_len = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    ext.array_join_rows(col.offsets.data_ptr(), placed.data_ptr(), dlen, n,
                        out_len.data_ptr(), s)
    out_off, nbytes = _exclusive_scan_i64(out_len)
    if nbytes > 2 ** 31 - 1:
        raise OverflowError("array_join result exceeds int32 offsets")
    out = torch.empty(max(nbytes, 1), **_NO_DATA)[:nbytes]
    ext.array_join_write(col.offsets.data_ptr(), _ptr(col.validity),
                         ch.offsets.data_ptr(), ch.data.data_ptr(),
                         _ptr(ch.validity), d.data_ptr(), dlen, r.data_ptr(),
                         rlen, placed.data_ptr(), out_off.data_ptr(), n,
                         out.data_ptr(), total if nbytes else 0, s)
    offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(out_off.data_ptr(), offs.data_ptr(), n + 1, s)
    return Column(DType.string(), n, out, v, offs, col._null_count)


def _array_extreme(col: Column, is_max: bool) -> Column:
    n = col.size
    s = _stream()
    elem = col.child
    if n == 0:
        return _empty_col(elem.dtype)
    off0, total, _, maxlen = _list_bounds(col)
    if total == 0:
        idx = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    else:
        t, dp, eo = _list_elem_args(elem)
        idx = torch.empty(n, dtype=torch.int32, device="cuda")
        ext.list_argminmax(t, dp, eo, _ptr(elem.validity),
                           col.offsets.data_ptr(), _ptr(col.validity),
                           _list_group_width(maxlen), is_max,
                           idx.data_ptr(), n, s)
    return _gather_col(elem, idx, n, maybe_negative=True)


def array_min(col: Column) -> Column:
    """Segmented arg-min over the sort keys (nulls skipped, NaN greatest),
    then a nullable gather of the child."""
    return _array_extreme(col, False)


def array_max(col: Column) -> Column:
    return _array_extreme(col, True)


def substring(col: Column, pos: int, length: int = -1) -> Column:
    n = col.size
    s = _stream()
    if n == 0:
        return _empty_col(DType.string())
    bstart = torch.empty(n, dtype=torch.int32, device="cuda")
    blen = torch.empty(n, dtype=torch.int64, device="cuda")
    ext.substr_ranges(col.offsets.data_ptr(), col.data.data_ptr(), pos,
                      length, bstart.data_ptr(), blen.data_ptr(), n, s)
    scanned, total = _exclusive_scan_i64(blen)
    out_bytes = torch.empty(max(total, 1), dtype=torch.uint8,
                            device="cuda")[:total]
    if total:
        ext.substr_copy(col.data.data_ptr(), bstart.data_ptr(),
                        blen.data_ptr(), scanned.data_ptr(),
                        out_bytes.data_ptr(), n, s)
    offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), n, s)
    offs[n] = total
    v = col.validity.clone() if col.validity is not None else None
    return Column(DType.string(), n, out_bytes, v, offs,
                  null_count=col._null_count)


def round_half_up(col: Column, scale: int) -> Column:
    return binary_op_scalar("round", col, float(10 ** scale), col.dtype)


def unary_op(op: str, col: Column, out_dtype: DType) -> Column:
    n = col.size
    s = _stream()
    if col.dtype.id is TypeId.STRING:
        v = col.validity.clone() if col.validity is not None else None
        if op == "length":
            out = _alloc(n, out_dtype)
            ext.str_length(col.offsets.data_ptr(), col.data.data_ptr(),
                           out.data_ptr(), n, s)
            return Column(out_dtype, n, out, v, null_count=col._null_count)
        if op in ("trim", "ltrim", "rtrim"):
            return str_trim(col, {"trim": "both", "ltrim": "leading",
                                  "rtrim": "trailing"}[op])
        if op in ("initcap", "reverse"):
            nb = int(col.data.numel())
            ob = torch.empty(max(nb, 1), dtype=torch.uint8,
                             device="cuda")[:nb]
            if n:
                fn = ext.str_initcap if op == "initcap" else ext.str_reverse
                fn(col.offsets.data_ptr(), col.data.data_ptr(),
                   ob.data_ptr(), n, s)
            return Column(out_dtype, n, ob, v, col.offsets.clone(),
                          null_count=col._null_count)
        if op in ("upper", "lower"):
            nb = int(col.data.numel())
            ob = torch.empty(max(nb, 1), dtype=torch.uint8,
                             device="cuda")[:nb]
            if nb:
                ext.str_case(op == "upper", col.data.data_ptr(),
                             ob.data_ptr(), nb, s)
            return Column(out_dtype, n, ob, v, col.offsets.clone(),
                          null_count=col._null_count)
        raise NotImplementedError(f"string unary {op} not on GPU")
    out = _alloc(n, out_dtype)
    if op in ("not", "is_nan", "year", "month", "day"):
        ext.unary(_UN_OPS[op], _ht(col.dtype), col.data.data_ptr(),
                  _ptr(col.validity), out.data_ptr(), 0, n, s)
        if op == "is_nan":
            return Column(out_dtype, n, out, None, null_count=0)
        v = col.validity.clone() if col.validity is not None else None
        return Column(out_dtype, n, out, v, null_count=col._null_count)
    need_mask = col.validity is not None or op == "log"
    ov = _alloc_mask(n) if need_mask else None
    ext.unary(_UN_OPS[op], _ht(col.dtype), col.data.data_ptr(),
              _ptr(col.validity), out.data_ptr(), _ptr(ov), n, s)
    return Column(out_dtype, n, out, ov, null_count=None if need_mask else 0)


def cast(col: Column, to: DType) -> Column:
    n = col.size
    s = _stream()
    v = col.validity.clone() if col.validity is not None else None
    if col.dtype.id is TypeId.STRING:
        # must run before the decimal branch: string -> decimal parses as
        # f64 first (truncating through int64 would drop the fraction)
        return _cast_string_to(col, to, v)
    if to.id is TypeId.STRING:
        return _cast_to_string(col, v)
    if col.dtype.is_decimal or to.is_decimal:
        return _cast_decimal(col, to, v)
    out = _alloc(n, to)
    ext.cast(_ht(col.dtype), _ht(to), col.data.data_ptr(), out.data_ptr(), n, s)
    return Column(to, n, out, v, null_count=col._null_count)


_STR_TO_KIND = {TypeId.INT8: 2, TypeId.INT16: 3, TypeId.INT32: 4,
                TypeId.INT64: 5}


def _cast_string_to(col: Column, to: DType, v) -> Column:
    """string -> numeric cast (CastStrings analogue). Integral and decimal
    targets parse EXACTLY on device (k_str_to_dec: u128 digit accumulate,
    HALF_UP for decimals, truncate-toward-zero for ints, null on
    overflow/garbage); float targets ride the CSV f64 parser."""
    n = col.size
    s = _stream()
    if to.is_decimal or to.is_integral:
        if to.id is TypeId.DECIMAL128:
            kind, scale, prec = 1, to.scale, to.precision
            width = 2 * n
        elif to.id is TypeId.DECIMAL64:
            kind, scale, prec = 0, to.scale, to.precision
            width = n
        else:
            kind, scale, prec = _STR_TO_KIND[to.id], 0, 39
            width = n
        out64 = torch.empty(max(width, 1), dtype=torch.int64,
                            device="cuda")[:width]
        ov = _alloc_mask(n)
        if n:
            ext.str_to_dec(col.offsets.data_ptr(), col.data.data_ptr(),
                           _ptr(v), kind, scale, prec, out64.data_ptr(),
                           ov.data_ptr(), n, s)
        if to.is_decimal or to.id is TypeId.INT64:
            return Column(to, n, out64, ov, null_count=None)
        narrow = _alloc(n, to)
        if n:
            ext.cast(4, _ht(to), out64.data_ptr(), narrow.data_ptr(), n, s)
        return Column(to, n, narrow, ov, null_count=None)
    if not to.is_floating:
        raise NotImplementedError(f"gpu cast string -> {to}")
    trimmed = str_trim(col, "cast")  # full ASCII whitespace (Spark casts)
    f64 = torch.empty(max(n, 1), dtype=torch.float64, device="cuda")[:n]
    valid_u8 = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")[:n]
    unsupported = torch.zeros(1, dtype=torch.int32, device="cuda")
    if n:
        ext.csv_parse(trimmed.data.data_ptr(),
                      trimmed.offsets[:n].data_ptr(),
                      trimmed.offsets[1:].data_ptr(), 0, 0, 1,
                      0, f64.data_ptr(), 0, 0, valid_u8.data_ptr(),
                      unsupported.data_ptr(), n, s)
    from ..column import mask_nbytes

    v64 = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")[:n]
    if n:
        ext.cast(0, 4, valid_u8.data_ptr(), v64.data_ptr(), n, s)
    pmask = torch.empty(mask_nbytes(n), dtype=torch.uint8, device="cuda")
    if n:
        ext.mask_from_nonzero(v64.data_ptr(), pmask.data_ptr(), n, s)
    mask = _and_masks(v, pmask) if v is not None else pmask
    wide = Column(DType.float64(), n, f64, mask, null_count=None)
    if to.id is TypeId.FLOAT64:
        return wide
    return cast(wide, to)


def _cast_to_string(col: Column, v) -> Column:
    """integral/decimal/date -> string on device; floats fall back (Java
    shortest-roundtrip float formatting parity is CPU-side, mirroring the
    reference's castFloatToString incompat gate)."""
    n = col.size
    s = _stream()
    if col.dtype.is_decimal:
        is128 = 1 if col.dtype.id is TypeId.DECIMAL128 else 0
        lens = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")[:n]
        if n:
            ext.dec_to_str(col.data.data_ptr(), is128, col.dtype.scale,
                           0, lens.data_ptr(), 0, 0, n, s)
        scanned, total = _exclusive_scan_i64(lens) if n else (lens, 0)
        out = torch.empty(max(total, 1), dtype=torch.uint8,
                          device="cuda")[:total]
        if total:
            ext.dec_to_str(col.data.data_ptr(), is128, col.dtype.scale,
                           scanned.data_ptr(), lens.data_ptr(),
                           out.data_ptr(), 1, n, s)
        offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
        if n:
            ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), n, s)
        offs[n] = total
        return Column(DType.string(), n, out, v, offs,
                      null_count=None if v is not None else 0)
    if not col.dtype.is_integral and col.dtype.id is not TypeId.BOOL:
        raise NotImplementedError(f"gpu cast {col.dtype} -> string")
    i64 = cast(Column(col.dtype, n, col.data, None, null_count=0),
               DType.int64()) if col.dtype.id is not TypeId.INT64         else Column(DType.int64(), n, col.data, None, null_count=0)
    lens = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")[:n]
    if n:
        ext.i64_to_str(i64.data.data_ptr(), 0, lens.data_ptr(), 0, 0, n, s)
    scanned, total = _exclusive_scan_i64(lens) if n else (lens, 0)
    out = torch.empty(max(total, 1), dtype=torch.uint8,
                      device="cuda")[:total]
    if total:
        ext.i64_to_str(i64.data.data_ptr(), scanned.data_ptr(),
                       lens.data_ptr(), out.data_ptr(), 1, n, s)
    offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    if n:
        ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), n, s)
    offs[n] = total
    return Column(DType.string(), n, out, v, offs,
                  null_count=None if v is not None else 0)


def _cast_decimal(col: Column, to: DType, v) -> Column:
    n = col.size
    s = _stream()
    if col.dtype.is_decimal and to.is_decimal:
        if to.scale == col.dtype.scale and to.id is col.dtype.id \
                and to.precision >= col.dtype.precision:
            # pure widening retype: no rescale, no overflow possible
            return Column(to, n, col.data.clone(), v,
                          null_count=col._null_count)
        # Widen to int128 FIRST, then rescale exactly in 128-bit with
        # HALF_UP down-shift and null-on-overflow (Spark non-ANSI).
        # Rescaling inside int64 before widening silently overflows
        # (decimal(18,0) + decimal(18,10)); the same
        # kernel checks the target precision for narrowing user casts.
        if col.dtype.id is TypeId.DECIMAL64:
            wide = torch.empty(max(2 * n, 1), dtype=torch.int64,
                               device="cuda")[:2 * n]
            if n:
                ext.i64_to_i128(col.data.data_ptr(), wide.data_ptr(), n, s)
            src128 = wide
        else:
            src128 = col.data
        shift = to.scale - col.dtype.scale
        out_is_64 = to.id is TypeId.DECIMAL64
        width = n if out_is_64 else 2 * n
        out = torch.empty(max(width, 1), dtype=torch.int64,
                          device="cuda")[:width]
        ov = _alloc_mask(n)
        if n:
            ext.i128_rescale(src128.data_ptr(), _ptr(v), out.data_ptr(),
                             ov.data_ptr(), shift, to.precision,
                             1 if out_is_64 else 0, n, s)
        return Column(to, n, out, ov, null_count=None)
    if col.dtype.id is TypeId.DECIMAL128 or to.id is TypeId.DECIMAL128:
        if col.dtype.id is TypeId.DECIMAL128 and to.is_floating:
            dbl = torch.empty(max(n, 1), dtype=torch.float64,
                              device="cuda")[:n]
            if n:
                ext.i128_to_f64(col.data.data_ptr(), dbl.data_ptr(), n, s)
            c = Column(DType.float64(), n, dbl, v, null_count=col._null_count)
            scaled = binary_op_scalar("div", c, float(10 ** col.dtype.scale),
                                      DType.float64())
            scaled = Column(DType.float64(), n, scaled.data, v,
                            null_count=col._null_count)
            return cast(scaled, to) if to.id is not TypeId.FLOAT64 else scaled
        if col.dtype.is_integral and to.id is TypeId.DECIMAL128:
            # integral -> decimal128: treat as decimal(scale 0) and rescale
            i64 = col if col.dtype.id is TypeId.INT64 \
                else cast(Column(col.dtype, n, col.data, None, null_count=0),
                          DType.int64())
            as_dec = Column(DType.decimal(18, 0), n, i64.data, v,
                            null_count=col._null_count)
            return _cast_decimal(as_dec, to, v)
        raise NotImplementedError(f"gpu cast {col.dtype} -> {to}")
    if col.dtype.is_decimal:
        # decimal -> float/int: via double divide
        dbl = _alloc(n, DType.float64())
        ext.cast(_ht(col.dtype), 6, col.data.data_ptr(), dbl.data_ptr(), n, s)
        c = Column(DType.float64(), n, dbl, v, null_count=col._null_count)
        scaled = binary_op_scalar("div", c, float(10 ** col.dtype.scale),
                                  DType.float64())
        scaled = Column(DType.float64(), n, scaled.data, v,
                        null_count=col._null_count)
        return cast(scaled, to) if to.id is not TypeId.FLOAT64 else scaled
    # numeric -> decimal: scale up in int64 (float sources rounded)
    i64 = cast(col, DType.int64()) if not col.dtype.is_floating else None
    if i64 is not None:
        out = _alloc(n, to)
        ext.decimal_rescale(i64.data.data_ptr(), out.data_ptr(),
                            10 ** to.scale, True, n, s)
        return Column(to, n, out, v, null_count=col._null_count)
    dbl = cast(col, DType.float64())
    scaled = binary_op_scalar("mul", dbl, float(10 ** to.scale),
                              DType.float64())
    out = _alloc(n, to)
    # round-to-nearest (not the truncating int cast): 40.5074 * 10^4 is
    # 405073.9999.. in binary and must become 405074
    ext.f64_to_i64_rint(scaled.data.data_ptr(), out.data_ptr(), n, s)
    return Column(to, n, out, v, null_count=col._null_count)


def is_null(col: Column) -> Column:
    n = col.size
    out = torch.zeros(max(n, 1), dtype=torch.uint8, device="cuda")[:n]
    if col.validity is not None and n:
        ext.mask_expand(col.validity.data_ptr(), out.data_ptr(), True, n,
                        _stream())
    return Column(DType.bool_(), n, out, None, null_count=0)


def if_else(cond: Column, a: Column, b: Column) -> Column:
    n = cond.size
    s = _stream()
    # cond-as-selector: rows where cond true+valid take a, else b
    out = _alloc(n, a.dtype) if a.dtype.id is not TypeId.STRING else None
    if out is None:
        raise NotImplementedError("if_else on strings not on GPU yet")
    ov = _alloc_mask(n)
    ext.if_else(_ht(a.dtype), cond.data.data_ptr(), _ptr(cond.validity),
                a.data.data_ptr(), _ptr(a.validity), b.data.data_ptr(),
                _ptr(b.validity), out.data_ptr(), ov.data_ptr(), n, s)
    has_valid = a.validity is not None or b.validity is not None
    return Column(a.dtype, n, out, ov if has_valid else None,
                  null_count=None if has_valid else 0)


# ---------------------------------------------------------------------------
# scan helper
# ---------------------------------------------------------------------------

def _exclusive_scan_i64(vals: torch.Tensor,
                        also: Optional[torch.Tensor] = None):
    """Returns (exclusive scan tensor, total). `also`, a small int64 device
    tensor, rides along in the one blocking readback of the total and comes
    back as a third item, a list."""
    n = vals.numel()
    s = _stream()
    if n == 0:
        return (vals, 0) if also is None else (vals, 0, also.tolist())
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    scratch = torch.empty(ext.scan_scratch_elems(n), dtype=torch.int64,
                          device="cuda")
    # every level in one native call; the grand total is scratch's last slot
    ext.exclusive_scan_i64(vals.data_ptr(), out.data_ptr(),
                           scratch.data_ptr(), n, s)
    if also is None:
        return out, int(scratch[-1].item())
    host = torch.cat([scratch[-1:], also]).tolist()
    return out, int(host[0]), host[1:]


# ---------------------------------------------------------------------------
# selection
# ---------------------------------------------------------------------------

def mask_to_sel(mask: Column, n: int) -> torch.Tensor:
    """Selection vector (int32 row indices) of rows where mask is true."""
    s = _stream()
    nb = ext.sel_num_blocks(n)
    counts = torch.empty(nb, dtype=torch.int64, device="cuda")
    ext.mask_count(mask.data.data_ptr(), _ptr(mask.validity),
                   counts.data_ptr(), n, s)
    offsets, total = _exclusive_scan_i64(counts)
    idx = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")[:total]
    if total:
        ext.mask_scatter(mask.data.data_ptr(), _ptr(mask.validity),
                         offsets.data_ptr(), idx.data_ptr(), n, s)
    return idx


def apply_boolean_mask(batch: ColumnBatch, mask: Column) -> ColumnBatch:
    idx = mask_to_sel(mask, batch.num_rows)
    return _gather_by_idx(batch, idx, idx.numel(), maybe_negative=False)


def gather(batch: ColumnBatch, indices: Column, check_bounds: bool = False,
           negatives: bool = True) -> ColumnBatch:
    return _gather_by_idx(batch, indices.data, indices.size,
                          maybe_negative=negatives)


def gather_dict(batch: ColumnBatch, indices: Column,
                negatives: bool = True) -> ColumnBatch:
    """gather() for a join's build side: STRING columns come back as
    dictionary views over the gather map instead of copied strings."""
    n_out = indices.size
    idx = indices.data
    if idx.numel() != n_out:
        idx = idx[:n_out]  # one tensor object: the views share their codes
    out = _gather_by_idx(batch, idx, n_out, maybe_negative=negatives,
                         dict_strings=True)
    # a non-null integer column gathered without misses holds a subset of
    # the build column's values: its range is found on the build column,
    # once for all probe batches (see _key_minmax), not per batch
    for src, c in zip(batch.columns, out.columns):
        if c.validity is None and c.dtype.id in _DENSE_OK \
                and not isinstance(c, DictColumn) and c.size:
            c._minmax = src
    return out


def _gather_validity(c: Column, idx: torch.Tensor,
                     n_out: int) -> torch.Tensor:
    ov = _alloc_mask(n_out)
    ext.gather_validity(_ptr(c.validity), c.validity is not None,
                        idx.data_ptr(), ov.data_ptr(), n_out, _stream())
    return ov


def _gather_view(c: DictColumn, idx: torch.Tensor, n_out: int,
                 maybe_negative: bool, shared: Optional[dict] = None
                 ) -> DictColumn:
    """Gather of a dictionary view: only the codes move, the result is a
    view over the same dictionary. `shared` maps id(codes) to the gathered
    codes, so views that shared their codes going in still do coming out
    (the group-by groups such keys jointly)."""
    codes = shared.get(id(c.codes)) if shared is not None else None
    if codes is None:
        codes = torch.empty(n_out, dtype=torch.int32, device="cuda")
        ext.gather_codes(c.codes.data_ptr(), idx.data_ptr(),
                         codes.data_ptr(), n_out, _stream())
        if shared is not None:
            shared[id(c.codes)] = codes
    return DictColumn(c.dictionary, codes, n_out,
                      c.maybe_negative or maybe_negative)


def _gather_col(c: Column, idx: torch.Tensor, n_out: int,
                maybe_negative: bool) -> Column:
    s = _stream()
    if n_out == 0:
        return _empty_col(c.dtype)
    if isinstance(c, DictColumn):
        return _gather_view(c, idx, n_out, maybe_negative)
    if c.dtype.id is TypeId.STRUCT:
        kids = tuple(_gather_col(k, idx, n_out, maybe_negative)
                     for k in c.child)
        ov = None
        if c.validity is not None or maybe_negative:
            ov = _alloc_mask(n_out)
            ext.gather_validity(_ptr(c.validity), c.validity is not None,
                                idx.data_ptr(), ov.data_ptr(), n_out, s)
        return Column(c.dtype, n_out,
                      torch.zeros(0, dtype=torch.uint8, device="cuda"),
                      ov, None, None if ov is not None else 0, kids)
    if c.dtype.id is TypeId.STRING:
        lens = torch.empty(n_out, dtype=torch.int64, device="cuda")
        ext.gather_str_lens(c.offsets.data_ptr(), idx.data_ptr(),
                            lens.data_ptr(), n_out, s)
        scanned, total = _exclusive_scan_i64(lens)
        out_bytes = torch.empty(max(total, 1), dtype=torch.uint8,
                                device="cuda")[:total]
        if total:
            ext.gather_str_bytes(c.data.data_ptr(), c.offsets.data_ptr(),
                                 idx.data_ptr(), scanned.data_ptr(),
                                 out_bytes.data_ptr(), n_out, total, s)
        offs = torch.empty(n_out + 1, dtype=torch.int32, device="cuda")
        ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), n_out, s)
        offs[n_out] = total
        ov = None
        if c.validity is not None or maybe_negative:
            ov = _alloc_mask(n_out)
            ext.gather_validity(_ptr(c.validity), c.validity is not None,
                                idx.data_ptr(), ov.data_ptr(), n_out, s)
        return Column(c.dtype, n_out, out_bytes, ov, offs, null_count=None if ov is not None else 0)
    out = _alloc(n_out, c.dtype)
    ext.gather_fixed(c.dtype.itemsize, c.data.data_ptr(), idx.data_ptr(),
                     out.data_ptr(), n_out, s)
    ov = None
    nc = 0
    if c.validity is not None or maybe_negative:
        ov = _alloc_mask(n_out)
        ext.gather_validity(_ptr(c.validity), c.validity is not None,
                            idx.data_ptr(), ov.data_ptr(), n_out, s)
        nc = None
    return Column(c.dtype, n_out, out, ov, null_count=nc)


def _gather_by_idx(batch: ColumnBatch, idx: torch.Tensor, n_out: int,
                   maybe_negative: bool,
                   dict_strings: bool = False) -> ColumnBatch:
    s = _stream()
    cols: List[Optional[Column]] = [None] * len(batch.columns)
    fixed: List[tuple] = []  # (position, column)
    shared: dict = {}  # gathered codes of the views, by id(source codes)
    for ci, c in enumerate(batch.columns):
        if isinstance(c, DictColumn) and n_out:
            # composes when `batch` is itself a join's build side
            cols[ci] = _gather_view(c, idx, n_out, maybe_negative, shared)
        elif dict_strings and c.dtype.id is TypeId.STRING and n_out:
            cols[ci] = DictColumn(c, idx, n_out, maybe_negative)
        elif c.dtype.id in (TypeId.STRING, TypeId.STRUCT) or n_out == 0:
            cols[ci] = _gather_col(c, idx, n_out, maybe_negative)
        else:
            fixed.append((ci, c))
    if fixed:
        blobs = []
        outs = []
        for ci, c in fixed:
            out = _alloc(n_out, c.dtype)
            need_valid = c.validity is not None or maybe_negative
            ov = _alloc_mask(n_out) if need_valid else None
            outs.append((ci, c, out, ov))
            # HipdfGatherCol (see native/hipdf/include/hipdf.h)
            blobs.append(struct.pack(
                "<iiqqqq", c.dtype.itemsize,
                1 if c.validity is not None else 0, c.data.data_ptr(),
                _ptr(c.validity), out.data_ptr(), _ptr(ov)))
        desc = torch.frombuffer(bytearray(b"".join(blobs)),
                                dtype=torch.uint8).cuda()
        ext.gather_table(desc.data_ptr(), len(fixed), idx.data_ptr(), n_out, s)
        for ci, c, out, ov in outs:
            cols[ci] = Column(c.dtype, n_out, out, ov,
                              null_count=None if ov is not None else 0)
            if ov is None:
                # a subset of c's rows: a range known for c holds here too
                cols[ci]._minmax = c._minmax
    return ColumnBatch(cols, n_out)


def concat_batches(batches: List[ColumnBatch]) -> ColumnBatch:
    s = _stream()
    total = sum(b.num_rows for b in batches)
    ncols = batches[0].num_columns
    out_cols = []
    cat_codes: dict = {}  # concatenated codes by the ids of their inputs
    for ci in range(ncols):
        ins = [b.columns[ci] for b in batches]
        if total and all(isinstance(c, DictColumn)
                         and c.dictionary is ins[0].dictionary for c in ins):
            # views over one dictionary: concatenate the codes, and keep
            # columns that shared their codes sharing them
            key = tuple(id(c.codes) for c in ins)
            if key not in cat_codes:
                cat_codes[key] = torch.cat([c.codes for c in ins])
            out_cols.append(DictColumn(
                ins[0].dictionary, cat_codes[key], total,
                any(c.maybe_negative for c in ins)))
            continue
        if ins[0].dtype.id is TypeId.LIST:
            raise NotImplementedError(
                "concat of LIST columns on GPU (explode or collect before "
                "unioning, or keep the union on the CPU)")
        dtype = ins[0].dtype
        if dtype.id is TypeId.STRUCT:
            any_valid = any(c.validity is not None for c in ins)
            out_valid = None
            if any_valid:
                out_valid = torch.zeros(mask_nbytes(total),
                                        dtype=torch.uint8, device="cuda")
                off = 0
                for c in ins:
                    if c.size:
                        ext.copy_valid_range(_ptr(c.validity),
                                             c.validity is not None, off,
                                             out_valid.data_ptr(), c.size,
                                             s)
                    off += c.size
            kids = tuple(
                concat_batches([ColumnBatch([c.child[k]], c.size)
                                for c in ins]).columns[0]
                for k in range(len(dtype.children)))
            out_cols.append(Column(
                dtype, total, torch.zeros(0, dtype=torch.uint8,
                                          device="cuda"),
                out_valid, None, None if any_valid else 0, kids))
            continue
        any_valid = any(c.validity is not None for c in ins)
        out_valid = None
        if any_valid:
            out_valid = torch.zeros(mask_nbytes(total), dtype=torch.uint8,
                                    device="cuda")
            off = 0
            for c in ins:
                if c.size:
                    ext.copy_valid_range(_ptr(c.validity),
                                         c.validity is not None, off,
                                         out_valid.data_ptr(), c.size, s)
                off += c.size
        if dtype.id is TypeId.STRING:
            data = torch.cat([c.data for c in ins])
            offs = torch.empty(total + 1, dtype=torch.int32, device="cuda")
            offs[0] = 0
            row_off, byte_off = 0, 0
            for c in ins:
                if c.size:
                    seg = offs[row_off + 1: row_off + 1 + c.size]
                    seg.copy_(c.offsets[1:c.size + 1])
                    if byte_off:
                        ext.binary_arith(_BIN_OPS["add"], 3, seg.data_ptr(),
                                         0, 0.0, byte_off, True, 0, 0,
                                         seg.data_ptr(), 0, c.size, s)
                row_off += c.size
                byte_off += int(c.data.numel())
            out_cols.append(Column(dtype, total, data, out_valid, offs,
                                   null_count=None if any_valid else 0))
        else:
            data = torch.cat([c.data for c in ins]) if total else \
                torch.zeros(0, dtype=torch_dtype(dtype), device="cuda")
            out_cols.append(Column(dtype, total, data, out_valid,
                                   null_count=None if any_valid else 0))
    return ColumnBatch(out_cols, total)


# ---------------------------------------------------------------------------
# hashing / partition
# ---------------------------------------------------------------------------

_HASH_KIND = {
    TypeId.BOOL: _HK_INT, TypeId.INT8: _HK_INT, TypeId.INT16: _HK_INT,
    TypeId.INT32: _HK_INT, TypeId.DATE32: _HK_INT,
    TypeId.INT64: _HK_LONG, TypeId.TIMESTAMP: _HK_LONG,
    TypeId.DECIMAL64: _HK_LONG,
    TypeId.FLOAT32: _HK_FLOAT, TypeId.FLOAT64: _HK_DOUBLE,
}


def _murmur3_tensor(cols: List[Column], seed: int,
                    sel: Optional[torch.Tensor] = None,
                    n_out: Optional[int] = None) -> torch.Tensor:
    n = cols[0].size if sel is None else (n_out if n_out is not None
                                          else sel.numel())
    s = _stream()
    seeds = torch.full((max(n, 1),), seed, dtype=torch.int32, device="cuda")[:n]
    selp = 0 if sel is None else sel.data_ptr()
    for c in cols:
        if n == 0:
            break
        if c.dtype.id is TypeId.STRING:
            ext.murmur3_str(c.offsets.data_ptr(), c.data.data_ptr(),
                            _ptr(c.validity), selp, seeds.data_ptr(), n, s)
        elif c.dtype.id is TypeId.DECIMAL128:
            ext.murmur3_col(5, 4, c.data.data_ptr(), _ptr(c.validity), selp,
                            seeds.data_ptr(), n, s)
        else:
            ext.murmur3_col(_HASH_KIND[c.dtype.id], _ht(c.dtype),
                            c.data.data_ptr(), _ptr(c.validity), selp,
                            seeds.data_ptr(), n, s)
    return seeds


def murmur3_hash(cols: List[Column], seed: int = 42) -> Column:
    h = _murmur3_tensor(cols, seed)
    return Column(DType.int32(), cols[0].size, h, None, null_count=0)


def hash_partition(batch: ColumnBatch, key_idx: List[int], num_parts: int):
    n = batch.num_rows
    s = _stream()
    if n == 0:
        return batch, [0] * (num_parts + 1)
    h = _murmur3_tensor([batch.columns[i] for i in key_idx], 42)
    part = torch.empty(n, dtype=torch.int32, device="cuda")
    ext.pmod_part(h.data_ptr(), num_parts, part.data_ptr(), n, s)
    perm, offsets = _scatter_by_part(part, n, num_parts)
    out = _gather_by_idx(batch, perm, n, maybe_negative=False)
    return out, offsets


def _scatter_by_part(part: torch.Tensor, n: int, num_parts: int):
    s = _stream()
    nb = ext.part_num_blocks(n)
    counts = torch.empty(num_parts * nb, dtype=torch.int64, device="cuda")
    ext.part_hist(part.data_ptr(), num_parts, counts.data_ptr(), n, s)
    scanned, _total = _exclusive_scan_i64(counts)
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    ext.part_scatter(part.data_ptr(), num_parts, scanned.data_ptr(),
                     perm.data_ptr(), n, s)
    # partition start offsets: exclusive scan of per-part totals
    per_part = counts.view(num_parts, nb).sum(dim=1).cpu().numpy()
    offs = np.zeros(num_parts + 1, dtype=np.int64)
    np.cumsum(per_part, out=offs[1:])
    return perm, offs.tolist()


# ---------------------------------------------------------------------------
# reduce
# ---------------------------------------------------------------------------

def reduce(op: str, col: Column):
    n = col.size
    if op == "count_all":
        return n
    if n == 0:
        return 0 if op == "count" else None
    s = _stream()
    is_f = col.dtype.is_floating
    if op == "mean":
        total = reduce("sum", col)
        cnt = reduce("count", col)
        return None if cnt == 0 else float(total) / cnt if total is not None else None
    init = {"sum": 0, "min": None, "max": None, "count": 0}[op]
    if is_f:
        acc = torch.full((1,), {"sum": 0.0, "min": float("inf"),
                                "max": float("-inf"), "count": 0.0}[op],
                         dtype=torch.float64, device="cuda")
    else:
        acc = torch.full((1,), {"sum": 0, "min": 2 ** 63 - 1,
                                "max": -2 ** 63, "count": 0}[op],
                         dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    if op == "count" and (not col.dtype.is_fixed_width
                          or col.dtype.id is TypeId.DECIMAL128):
        # count over STRING/nested/decimal128 (two words a row, no typed
        # accumulator): only the validity matters
        nn8 = torch.ones(max(n, 1), dtype=torch.uint8, device="cuda")[:n]
        col = Column(DType.bool_(), n, nn8, col.validity,
                     null_count=col._null_count)
    ext.reduce(_RED.get(op, 0), _ht(col.dtype), col.data.data_ptr(),
               _ptr(col.validity), acc.data_ptr(), cnt.data_ptr(), n, s)
    c = int(cnt.item())
    if op == "count":
        return c
    if c == 0:
        return None
    v = acc.item()
    if not is_f and col.dtype.id not in (TypeId.DECIMAL64,):
        v = int(v)
    return v


# ---------------------------------------------------------------------------
# group-by aggregate
# ---------------------------------------------------------------------------

def _key_desc(cols: List[Column]) -> torch.Tensor:
    """Pack HipdfKeyCol structs (see native/hipdf/include/hipdf.h) into
    device mem: {int type; int is_string; void* data; u64* valid; void* aux}
    = 32 B."""
    blobs = []
    for c in cols:
        if c.dtype.id is TypeId.STRING:
            blobs.append(struct.pack("<iiqqq", 0, 1, c.offsets.data_ptr(),
                                     _ptr(c.validity), c.data.data_ptr()))
        elif c.dtype.id is TypeId.DECIMAL128:
            blobs.append(struct.pack("<iiqqq", 7, 0, c.data.data_ptr(),
                                     _ptr(c.validity), 0))
        else:
            blobs.append(struct.pack("<iiqqq", _ht(c.dtype), 0,
                                     c.data.data_ptr(), _ptr(c.validity), 0))
    host = torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8)
    return host.cuda()


def _next_pow2(x: int) -> int:
    p = 1
    while p < x:
        p <<= 1
    return p


def group_by_aggregate(batch: ColumnBatch, key_idx: List[int],
                       aggs: List[Tuple[str, int, DType]],
                       sel: Optional[torch.Tensor] = None) -> ColumnBatch:
    """Hash group-by; with `sel` (int32 row indices) only the selected rows
    participate — the filter-into-aggregate fusion path (no materialized
    gather of the filtered batch)."""
    n = batch.num_rows if sel is None else sel.numel()
    s = _stream()
    keys = [batch.columns[i] for i in key_idx]
    if n == 0 and key_idx:
        out = [_empty_col(k.dtype) for k in keys]
        out += [_empty_col(dt) for _, _, dt in aggs]
        return ColumnBatch(out, 0)
    selp = 0 if sel is None else sel.data_ptr()
    dense = None
    if not key_idx:
        # global aggregate: single group
        row_gid = torch.zeros(n, dtype=torch.int32, device="cuda")
        ngroups = 1
        leaders = torch.zeros(1, dtype=torch.int32, device="cuda")
    elif (dense := _try_dense_keys(keys, aggs, selp, n)) is not None:
        # dense fast path: gid = radix index over small integer ranges and
        # over the group tables of dictionary-view keys — no hash table, no
        # probe and no string at this row count (k_dense_gid); empty ids
        # are compacted after aggregation
        row_gid, ngroups, dense_info = dense
        leaders = None
    else:
        # today's path over materialised strings; the result's key columns
        # are ordinary columns, not views of the views
        keys = [Column(k.dtype, k.size, k.data, k.validity, k.offsets,
                       k._null_count) if isinstance(k, DictColumn) else k
                for k in keys]
        row_gid, ngroups, leaders = _hash_group_ids(keys, sel, n)
    if leaders is not None:
        leaders = leaders[:ngroups]
    # leaders are ORIGINAL row ids (pre-selection), so gather keys from the
    # full-length key columns (hash path; the dense path reconstructs keys
    # arithmetically after compaction)
    key_batch = _gather_by_idx(ColumnBatch(keys, keys[0].size), leaders,
                               ngroups, maybe_negative=False) \
        if keys and leaders is not None else None
    out_cols = list(key_batch.columns) if key_batch is not None else []

    # fused multi-aggregate: one kernel pass accumulates every agg;
    # decimal128 sums go through dedicated carry-correct i128 kernels
    # replica count for the non-LDS atomic path: spreads a skew-hot
    # group's atomics over nrep accumulator copies (zipf keys would
    # otherwise serialize millions of atomics on one address)
    nrep = 1 if ngroups * max(1, len(aggs)) <= 4096 \
        else max(1, min(64, (1 << 21) // ngroups))
    allocs = []
    blobs = []
    for op, vidx, out_dtype in aggs:
        vc = batch.columns[vidx] if vidx >= 0 else None
        if op == "sum" and out_dtype.id is TypeId.DECIMAL128:
            acc = torch.zeros(2 * max(ngroups, 1), dtype=torch.int64,
                              device="cuda")
            cnt = torch.zeros(max(ngroups, 1), dtype=torch.int64,
                              device="cuda")
            if n:
                in64 = 0 if vc.dtype.id is TypeId.DECIMAL128 else 1
                if ngroups <= 2048:
                    # LDS-staged: one global flush per block instead of
                    # per-row atomics on a few hot accumulators
                    ext.gb_sum_i128_lds(
                        in64, vc.data.data_ptr(), _ptr(vc.validity),
                        row_gid.data_ptr(), selp, acc.data_ptr(),
                        cnt.data_ptr(), ngroups, n, s)
                elif in64:
                    ext.gb_sum_i64_to_i128(
                        vc.data.data_ptr(), _ptr(vc.validity),
                        row_gid.data_ptr(), selp, acc.data_ptr(),
                        cnt.data_ptr(), n, s)
                else:
                    ext.gb_sum_i128(vc.data.data_ptr(), _ptr(vc.validity),
                                    row_gid.data_ptr(), selp, acc.data_ptr(),
                                    cnt.data_ptr(), n, s)
            allocs.append(("sum_d128", out_dtype, False, acc, cnt, 0))
            continue
        if op in ("collect_list", "collect_set"):
            col = _gb_collect(vc, row_gid, selp, n, ngroups, out_dtype,
                              op == "collect_set", s)
            allocs.append(("collect", out_dtype, False, col, None, 0))
            continue
        if op.startswith("percentile:"):
            col = _gb_percentile(vc, row_gid, selp, n, ngroups,
                                 float(op.split(":", 1)[1]), s)
            allocs.append(("collect", out_dtype, False, col, None, 0))
            continue
        if op.startswith("hll:"):
            col = _gb_hll(vc, row_gid, selp, n, ngroups,
                          int(op.split(":", 1)[1]), s)
            allocs.append(("collect", out_dtype, False, col, None, 0))
            continue
        if op in ("min", "max") and vc is not None \
                and vc.dtype.id is TypeId.STRING:
            col = _gb_minmax_str(vc, row_gid, sel, n, ngroups,
                                 op == "max", s)
            allocs.append(("collect", out_dtype, False, col, None, 0))
            continue
        if op == "count" and vc is not None and (
                not vc.dtype.is_fixed_width
                or vc.dtype.id is TypeId.DECIMAL128):
            # count over STRING/nested/decimal128 only needs the validity:
            # swap in a u8 non-null indicator column so no typed
            # accumulator is hit
            nn8 = torch.ones(max(vc.size, 1), dtype=torch.uint8,
                             device="cuda")[:vc.size]
            vc = Column(DType.bool_(), vc.size, nn8, vc.validity,
                        null_count=vc._null_count)
        acc_is_double = out_dtype.is_floating or (
            vc is not None and vc.dtype.is_floating)
        acc = torch.empty(max(nrep * ngroups, 1),
                          dtype=torch.float64 if acc_is_double else torch.int64,
                          device="cuda")
        cnt = torch.zeros(max(nrep * ngroups, 1), dtype=torch.int64,
                          device="cuda")
        t = _ht(vc.dtype) if vc is not None else 4
        if op not in ("count", "count_all"):
            ext.gb_acc_init(_GB[op], acc.data_ptr(), acc_is_double,
                            nrep * ngroups, s)
        # sum / integer min-max over a non-null column: group validity
        # is implied by group existence, so the per-row count atomic is
        # pure traffic (roofline: k_gb_agg_multi writes were ~2x the
        # accumulator data). FLOAT min/max keep the count: the replica
        # fold needs it to tell an empty replica's ±inf init from a real
        # ±inf when NaN values are present (Spark: NaN is greatest).
        skip_cnt = 1 if (vc is not None and vc.validity is None and n > 0
                         and (op == "sum"
                              or (op in ("min", "max")
                                  and not vc.dtype.is_floating))) else 0
        allocs.append((op, out_dtype, acc_is_double, acc, cnt,
                       skip_cnt))
        # HipdfAggDesc (see native/hipdf/include/hipdf.h)
        blobs.append(struct.pack(
            "<iiiiqqqq", _GB[op], t, acc_is_double, skip_cnt,
            _ptr(vc.data if vc is not None else None),
            _ptr(vc.validity if vc is not None else None),
            acc.data_ptr(), cnt.data_ptr()))
    if blobs:
        desc = torch.frombuffer(bytearray(b"".join(blobs)),
                                dtype=torch.uint8).cuda()
        ext.gb_agg_multi(desc.data_ptr(), len(blobs), row_gid.data_ptr(),
                         selp, ngroups, nrep, n, s)
        if nrep > 1:
            for op, _, acc_is_double, acc, cnt, _skip in allocs:
                if op in ("sum_d128", "collect"):
                    continue
                ext.gb_reduce_reps(_GB.get(op, 0), acc.data_ptr(),
                                   1 if acc_is_double else 0,
                                   cnt.data_ptr(), ngroups, nrep, s)
    for op, out_dtype, acc_is_double, acc, cnt, skip_cnt in allocs:
        if op == "collect":
            out_cols.append(acc)
            continue
        if op == "sum_d128":
            ov = _alloc_mask(ngroups)
            ext.mask_from_nonzero(cnt.data_ptr(), ov.data_ptr(), ngroups, s)
            out_cols.append(Column(out_dtype, ngroups, acc[:2 * ngroups],
                                   ov, null_count=None))
            continue
        if op in ("count", "count_all"):
            out_cols.append(Column(out_dtype, ngroups, cnt[:ngroups].clone(),
                                   None, null_count=0))
            continue
        acc_dt = DType.float64() if acc_is_double else DType.int64()
        data = acc[:ngroups]
        if torch_dtype(out_dtype) != data.dtype:
            out_data = _alloc(ngroups, out_dtype)
            ext.cast(_ht(acc_dt), _ht(out_dtype), data.data_ptr(),
                     out_data.data_ptr(), ngroups, s)
        else:
            out_data = data
        if skip_cnt:
            # every observed group has >= 1 contributing row
            out_cols.append(Column(out_dtype, ngroups, out_data, None,
                                   null_count=0))
        else:
            ov = _alloc_mask(ngroups)
            ext.mask_from_nonzero(cnt.data_ptr(), ov.data_ptr(), ngroups, s)
            out_cols.append(Column(out_dtype, ngroups, out_data, ov,
                                   null_count=None))
    if dense is not None:
        return _compact_dense(out_cols, allocs, keys, dense_info, ngroups,
                              row_gid, n, s)
    return ColumnBatch(out_cols, ngroups)


_DENSE_OK = {TypeId.BOOL, TypeId.INT8, TypeId.INT16, TypeId.INT32,
             TypeId.INT64, TypeId.DATE32}


def _hash_group_ids(keys, sel, n):
    """Hash path: (row_gid[n], ngroups, leaders) with one leader row (an
    ORIGINAL row id, pre-selection) per group."""
    s = _stream()
    selp = 0 if sel is None else sel.data_ptr()
    h = _murmur3_tensor(keys, 42, sel, n)
    cap = max(1024, _next_pow2(2 * n))
    desc = _key_desc(keys)
    slot_row = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    row_slot = torch.empty(n, dtype=torch.int32, device="cuda")
    claimed = torch.empty(n, dtype=torch.int32, device="cuda")
    ngroups_t = torch.zeros(1, dtype=torch.int32, device="cuda")
    ext.gb_build(h.data_ptr(), desc.data_ptr(), len(keys), selp,
                 slot_row.data_ptr(), row_slot.data_ptr(),
                 claimed.data_ptr(), ngroups_t.data_ptr(), cap, n, s)
    slot_gid = torch.empty(cap, dtype=torch.int32, device="cuda")
    leaders = torch.empty(n, dtype=torch.int32, device="cuda")
    ext.gb_number(claimed.data_ptr(), slot_row.data_ptr(),
                  slot_gid.data_ptr(), ngroups_t.data_ptr(),
                  leaders.data_ptr(), n, s)
    ngroups = int(ngroups_t.item())
    row_gid = torch.empty(n, dtype=torch.int32, device="cuda")
    ext.gb_rowgid(row_slot.data_ptr(), slot_gid.data_ptr(),
                  row_gid.data_ptr(), n, s)
    return row_gid, ngroups, leaders


def _dict_group_table(dicts: List[Column], need_null_slot: bool):
    """Group the rows of the dictionary columns `dicts` (one dimension's
    columns, grouped jointly) with the hash path, at dimension scale.
    Returns (table, G, leaders, has_null_slot): table[r] is the group of
    dictionary row r in [0, G), leaders[g] one dictionary row of group g.
    With a NULL slot, slot G stands for "every key NULL": rows coded -1 go
    there, and so do dictionary rows whose strings are all NULL, so that
    both kinds of NULL key make one group (leaders[G] = -1).

    The result is cached on the leading dictionary column: the dictionaries
    are a join's build columns, the same objects for every probe batch, so a
    dimension's key strings are grouped once per query and not once per
    batch. The entry holds the other dictionaries, which keeps their ids
    from being reused, and nothing writes to the tensors it returns."""
    key = (tuple(id(c) for c in dicts), bool(need_null_slot))
    cache = dicts[0]._group_tables
    if cache is None:
        cache = dicts[0]._group_tables = {}
    hit = cache.get(key)
    if hit is None:
        hit = cache[key] = (list(dicts),
                            _build_dict_group_table(dicts, need_null_slot))
    return hit[1]


def _build_dict_group_table(dicts: List[Column], need_null_slot: bool):
    d = dicts[0].size
    if d == 0:
        table = torch.zeros(0, dtype=torch.int32, device="cuda")
        leaders = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        return table, 0, leaders, True
    table, g, leaders = _hash_group_ids(dicts, None, d)
    all_null_rows = all(c.validity is not None for c in dicts)
    if all_null_rows:
        ext.dense_null_slot(table.data_ptr(), _key_desc(dicts).data_ptr(),
                            len(dicts), g, d, _stream())
    has_null_slot = need_null_slot or all_null_rows
    leaders = leaders[:g]
    if has_null_slot:
        leaders = torch.cat([leaders, torch.full(
            (1,), -1, dtype=torch.int32, device="cuda")])
    return table, g, leaders, has_null_slot


def _column_minmax(k: Column):
    """(min, max) of a column: two reductions with a readback each."""
    return reduce("min", k), reduce("max", k)


def _key_minmax(k: Column):
    """A range that holds every value of the non-null integer key `k`,
    cached on the column: stored tables are re-scanned every query, and
    columns are immutable by convention. A column that a join gathered from
    its build side carries that build column in `_minmax` (gather_dict) and
    takes its range, which is found once on the build column, at dimension
    scale, however many probe batches there are. Such a range may be wider
    than the key's own; the dense ids only need it to cover the values."""
    mm = k._minmax
    if isinstance(mm, Column):
        mm = k._minmax = _key_minmax(mm)
    elif mm is None:
        mm = k._minmax = _column_minmax(k)
    return mm


def _try_dense_keys(keys, aggs, selp, n):
    """Dense path applicability: every key is a non-null small-range
    integer or a dictionary view, and the product of the ranges stays tiny
    relative to n. Views that share their codes (columns of one dimension)
    form one radix component, grouped jointly at dimension scale."""
    ints = [k for k in keys if not isinstance(k, DictColumn)]
    if any(k.dtype.id not in _DENSE_OK for k in ints):
        return None
    if any(k.validity is not None for k in ints):
        return None
    if any(op in ("collect_list", "collect_set") for op, _, _ in aggs):
        return None  # LIST columns cannot be re-gathered in compaction
    # components in key order: ("int", [pos], kmin, range) or
    # ("dict", [pos...], codes) for the views sharing one codes tensor
    comps: List[list] = []
    by_codes: dict = {}
    for i, k in enumerate(keys):
        if isinstance(k, DictColumn):
            comp = by_codes.get(id(k.codes))
            if comp is None:
                comp = by_codes[id(k.codes)] = ["dict", [], k.codes]
                comps.append(comp)
            comp[1].append(i)
            continue
        kmin, kmax = _key_minmax(k)
        if kmin is None:
            return None
        rng = int(kmax) - int(kmin) + 1
        if rng <= 0:
            return None
        comps.append(["int", [i], int(kmin), rng])
    limit = min(1 << 24, max(1 << 16, 4 * n))
    prod = 1
    for comp in comps:
        if comp[0] == "int":
            prod *= comp[3]
            if prod > limit:
                return None
    sizes = []
    for comp in comps:
        if comp[0] == "int":
            sizes.append(comp[3])
            continue
        views = [keys[i] for i in comp[1]]
        table, g, leaders, has_null = _dict_group_table(
            [v.dictionary for v in views],
            any(v.maybe_negative for v in views))
        comp.extend([table, g, leaders, has_null])
        sizes.append(g + (1 if has_null else 0))
        prod *= sizes[-1]
        if prod > limit:
            return None
    strides = [0] * len(comps)
    acc = 1
    for i in range(len(comps) - 1, -1, -1):
        strides[i] = acc
        acc *= sizes[i]
    s = _stream()
    # HipdfDenseKey (see native/hipdf/include/hipdf.h)
    blobs = []
    for comp, stride in zip(comps, strides):
        if comp[0] == "int":
            k = keys[comp[1][0]]
            blobs.append(struct.pack("<iiqqqqqq", _ht(k.dtype), 0,
                                     k.data.data_ptr(), 0, comp[2], comp[3],
                                     stride, 0))
        else:
            blobs.append(struct.pack("<iiqqqqqq", 3, 0, comp[3].data_ptr(),
                                     0, 0, comp[4], stride,
                                     comp[2].data_ptr()))
    desc = torch.frombuffer(bytearray(b"".join(blobs)),
                            dtype=torch.uint8).cuda()
    row_gid = torch.empty(n, dtype=torch.int32, device="cuda")
    # without a count_all aggregate the compaction learns the live ids from
    # flags set in this same pass instead of counting every row again
    live = None
    if not any(op == "count_all" for op, _, _ in aggs):
        live = torch.zeros(max(prod, 1), dtype=torch.uint8, device="cuda")
    ext.dense_gid(desc.data_ptr(), len(comps), selp, row_gid.data_ptr(),
                  _ptr(live), n, s)
    return row_gid, prod, (comps, sizes, strides, live)


def _compact_dense(out_cols, allocs, keys, dense_info, ngroups, row_gid,
                   n, s):
    """Drop empty dense group ids and reconstruct the key columns from the
    surviving ids: an integer key is kmin + (g // stride) % range, a
    dictionary key a gather of its dictionary by the leader row of group
    (g // stride) % size, at result scale."""
    comps, sizes, strides, live_flags = dense_info
    if live_flags is not None:
        live = Column(DType.bool_(), ngroups, live_flags[:ngroups], None,
                      null_count=0)
    else:
        counts = next(cnt for (op, _, _, _acc, cnt, _sk) in allocs
                      if op == "count_all")
        ccol = Column(DType.int64(), ngroups, counts[:ngroups], None,
                      null_count=0)
        live = binary_op_scalar("gt", ccol, 0, DType.bool_())
    gsel = mask_to_sel(live, ngroups)
    ncomp = gsel.numel()
    gcol = Column(DType.int32(), ncomp, gsel, None, null_count=0)
    g64 = cast(gcol, DType.int64())
    key_cols: List[Optional[Column]] = [None] * len(keys)
    for i, comp in enumerate(comps):
        code = g64
        if strides[i] != 1:
            code = binary_op_scalar("int_div", code, strides[i],
                                    DType.int64())
        if i > 0:  # leading key needs no modulo (gid < stride_{i-1}*range)
            code = binary_op_scalar("mod", code, sizes[i], DType.int64())
        if comp[0] == "int":
            if comp[2]:
                code = binary_op_scalar("add", code, comp[2], DType.int64())
            key_cols[comp[1][0]] = cast(code, keys[comp[1][0]].dtype)
            continue
        leaders, has_null = comp[5], comp[6]
        if ncomp == 0:
            for pos in comp[1]:
                key_cols[pos] = _empty_col(keys[pos].dtype)
            continue
        slot = cast(code, DType.int32())
        rows = torch.empty(ncomp, dtype=torch.int32, device="cuda")
        ext.gather_codes(leaders.data_ptr(), slot.data.data_ptr(),
                         rows.data_ptr(), ncomp, s)
        for pos in comp[1]:
            key_cols[pos] = _gather_col(keys[pos].dictionary, rows, ncomp,
                                        maybe_negative=has_null)
    agg_batch = _gather_by_idx(ColumnBatch(out_cols, ngroups), gsel, ncomp,
                               maybe_negative=False)
    return ColumnBatch(key_cols + list(agg_batch.columns), ncomp)


def _gb_collect_str(vc: Column, row_gid: torch.Tensor, selp, n: int,
                    ngroups: int, out_dtype, s) -> Column:
    """collect_list over strings: stable-sort rows by group id, then one
    string gather in group order; offsets come from the per-group valid
    counts."""
    if selp:
        raise NotImplementedError("string collect under filter fusion")
    # drop null values first (collect skips nulls) while keeping gids
    gid_col = Column(DType.int32(), n, row_gid[:n], None, null_count=0)
    if vc.validity is not None:
        nn = unary_op("not", is_null(vc), DType.bool_())
        kept = apply_boolean_mask(ColumnBatch([gid_col, vc], n), nn)
        gid_col, vc = kept.columns[0], kept.columns[1]
        n = kept.num_rows
    pair = ColumnBatch([gid_col, vc], n)
    perm = sort_order(pair, [0], [False], [False])
    child = _gather_col(vc, perm.data, n, maybe_negative=False)
    counts = torch.zeros(max(ngroups, 1), dtype=torch.int64, device="cuda")
    if n:
        ext.gb_collect_count(0, gid_col.data.data_ptr(), 0,
                             counts.data_ptr(), n, s)
    scanned, total = _exclusive_scan_i64(counts[:ngroups]) if ngroups \
        else (counts, 0)
    offs = torch.empty(ngroups + 1, dtype=torch.int32, device="cuda")
    if ngroups:
        ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), ngroups, s)
    offs[ngroups] = total
    return Column(out_dtype, ngroups, torch.zeros(0, dtype=torch.uint8,
                                                  device="cuda"),
                  None, offs, 0, child)


def _gb_percentile(vc: Column, row_gid: torch.Tensor, selp, n: int,
                   ngroups: int, p: float, s) -> Column:
    """Exact percentile (linear interpolation): sort (gid, value) with
    nulls last, then interpolate inside each group's valid window
    (k_gb_percentile). Reference analogue: GpuPercentile."""
    if selp:
        raise NotImplementedError("percentile under filter fusion")
    vf = cast(vc, DType.float64()) if vc.dtype.id is not TypeId.FLOAT64 \
        else vc
    gid_col = Column(DType.int32(), n, row_gid[:n], None, null_count=0)
    pair = ColumnBatch([gid_col, vf], n)
    perm = sort_order(pair, [0, 1], [False, False], [True, True])
    total = torch.zeros(max(ngroups, 1), dtype=torch.int64, device="cuda")
    vcnt = torch.zeros(max(ngroups, 1), dtype=torch.int64, device="cuda")
    if n:
        ext.gb_collect_count(0, row_gid.data_ptr(), 0, total.data_ptr(),
                             n, s)
        ext.gb_collect_count(_ptr(vf.validity), row_gid.data_ptr(), 0,
                             vcnt.data_ptr(), n, s)
    starts, _ = _exclusive_scan_i64(total[:ngroups]) if ngroups \
        else (total, 0)
    out = torch.empty(max(ngroups, 1), dtype=torch.float64,
                      device="cuda")[:ngroups]
    if ngroups:
        ext.gb_percentile(vf.data.data_ptr(), perm.data.data_ptr(),
                          starts.data_ptr(), vcnt.data_ptr(), p,
                          out.data_ptr(), ngroups, s)
    ov = _alloc_mask(ngroups)
    ext.mask_from_nonzero(vcnt.data_ptr(), ov.data_ptr(), ngroups, s)
    return Column(DType.float64(), ngroups, out, ov, null_count=None)


def _gb_minmax_str(vc: Column, row_gid: torch.Tensor, sel, n: int,
                   ngroups: int, is_max: bool, s) -> Column:
    """min/max over STRING values per group, sort-based: stable radix
    sort of (gid, value) (string keys via the chunked big-endian LSD
    machinery), then the head row of each gid segment is the extreme.
    Nulls sort last so any non-null wins; an all-null group's head is a
    null row and gathers as NULL (Spark ignore-null semantics)."""
    gid_col = Column(DType.int32(), n, row_gid[:n], None, null_count=0)
    if sel is not None:
        vals = _gather_col(vc, sel, n, maybe_negative=False)
    else:
        vals = vc
    pair = ColumnBatch([gid_col, vals], n)
    perm = sort_order(pair, [0, 1], [False, is_max], [False, True])
    pg = perm.data[:n].long()
    sg = row_gid[:n].long()[pg] if sel is None else \
        row_gid[:n].long()[pg]
    head = torch.ones(n, dtype=torch.bool, device="cuda")
    if n > 1:
        head[1:] = sg[1:] != sg[:-1]
    hp = head.nonzero(as_tuple=True)[0]
    orig = pg[hp] if sel is None else sel[:n].long()[pg[hp]]
    ridx = torch.full((ngroups,), -1, dtype=torch.int32, device="cuda")
    ridx[sg[hp]] = orig.to(torch.int32)
    return _gather_col(vc, ridx, ngroups, maybe_negative=True)


def _gb_collect(vc: Column, row_gid: torch.Tensor, selp, n: int,
                ngroups: int, out_dtype, is_set: bool, s) -> Column:
    """collect_list/collect_set: count-per-group + scan + atomic-cursor
    scatter (k_gb_collect_* in groupby.hip). collect_set dedupes first by
    grouping the (gid, value) pairs with the generic hash groupby."""
    elem_dt = out_dtype.children[0]
    if elem_dt.id is TypeId.STRING and not is_set:
        return _gb_collect_str(vc, row_gid, selp, n, ngroups, out_dtype, s)
    if is_set:
        if selp:
            raise NotImplementedError(
                "collect_set under filter fusion: the single-pass exec "
                "path materializes filtered batches, so sel is never set")
        # dedupe the (gid, value) pairs with the generic hash groupby, then
        # collect the unique pairs using gid as a direct group index
        gid_col = Column(DType.int32(), n, row_gid[:n], None, null_count=0)
        pair = ColumnBatch([gid_col, vc], n)
        uniq = group_by_aggregate(pair, [0, 1], [])
        ug, uv = uniq.columns[0], uniq.columns[1]
        return _gb_collect(uv, ug.data[:uniq.num_rows], None,
                           uniq.num_rows, ngroups, out_dtype, False, s)
    counts = torch.zeros(max(ngroups, 1), dtype=torch.int64, device="cuda")
    if n:
        ext.gb_collect_count(_ptr(vc.validity), row_gid.data_ptr(),
                             selp or 0, counts.data_ptr(), n, s)
    scanned, total = _exclusive_scan_i64(counts[:ngroups]) if ngroups         else (counts, 0)
    esize = 16 if elem_dt.id is TypeId.DECIMAL128 else         torch.empty(0, dtype=torch_dtype(elem_dt)).element_size()
    nelem = 2 * total if elem_dt.id is TypeId.DECIMAL128 else total
    out_data = torch.empty(max(nelem, 1), dtype=torch_dtype(elem_dt),
                           device="cuda")[:nelem]
    cursor = torch.zeros(max(ngroups, 1), dtype=torch.int64, device="cuda")
    if n and total:
        ext.gb_collect_fill(esize, vc.data.data_ptr(), _ptr(vc.validity),
                            row_gid.data_ptr(), selp or 0,
                            scanned.data_ptr(), cursor.data_ptr(),
                            out_data.data_ptr(), n, s)
    offs = torch.empty(ngroups + 1, dtype=torch.int32, device="cuda")
    if ngroups:
        ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), ngroups, s)
    offs[ngroups] = total
    child = Column(elem_dt, total, out_data, None, null_count=0)
    return Column(out_dtype, ngroups, torch.zeros(0, dtype=torch.uint8,
                                                  device="cuda"),
                  None, offs, 0, child)


# ---------------------------------------------------------------------------
# join
# ---------------------------------------------------------------------------

_JOIN_SEED = 42  # JOIN_SEED in native/hipdf/kernels/join.hip


class JoinTable:
    """Chained hash table over the build side of an equi-join, built once
    and probed by every left batch. `unique` says no two non-null build rows
    share a key, which lets the probe take the single-pass path."""

    __slots__ = ("keys", "desc", "hashes", "head", "next", "cap", "num_rows",
                 "unique")

    def __init__(self, keys, desc, hashes, head, nxt, cap, num_rows, unique):
        self.keys = keys          # build key columns (keeps buffers alive)
        self.desc = desc          # device KeyCol descriptors of the keys
        self.hashes = hashes      # murmur3 row hashes of the build keys
        self.head = head
        self.next = nxt
        self.cap = cap
        self.num_rows = num_rows
        self.unique = unique


def join_build_table(right: ColumnBatch, right_keys: List[int]) -> JoinTable:
    s = _stream()
    nr = right.num_rows
    rk = [right.columns[i] for i in right_keys]
    cap = max(1024, _next_pow2(2 * max(nr, 1)))
    rh = _murmur3_tensor(rk, _JOIN_SEED)
    rdesc = _key_desc(rk)
    head = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    nxt = torch.empty(max(nr, 1), dtype=torch.int32, device="cuda")
    ext.join_build(rh.data_ptr(), rdesc.data_ptr(), len(rk), head.data_ptr(),
                   nxt.data_ptr(), cap, nr, s)
    unique = True
    if nr > 1:
        dup = torch.zeros(1, dtype=torch.int32, device="cuda")
        ext.join_check_unique(rdesc.data_ptr(), len(rk), nxt.data_ptr(),
                              dup.data_ptr(), nr, s)
        unique = int(dup.item()) == 0
    return JoinTable(rk, rdesc, rh, head, nxt, cap, nr, unique)


def _join_inline_key_type(lk: List[Column], rk: List[Column]) -> int:
    """HType of the key when the probe can hash it inline (one integer key
    column of the same type on both sides), else -1."""
    if len(lk) != 1 or lk[0].dtype.id is not rk[0].dtype.id:
        return -1
    if _HASH_KIND.get(lk[0].dtype.id) not in (_HK_INT, _HK_LONG):
        return -1
    return _ht(lk[0].dtype)


_ARANGE_I32: dict = {}  # device index -> cached int32 arange


def _identity_map(n: int) -> torch.Tensor:
    """Read-only view of a cached int32 arange (the left map of a left/full
    join against a unique build side). Callers only gather through it."""
    dev = torch.cuda.current_device()
    cached = _ARANGE_I32.get(dev)
    if cached is None or cached.numel() < n:
        cached = torch.arange(max(n, 1 << 20), dtype=torch.int32,
                              device="cuda")
        # the cache outlives the stream that filled it
        torch.cuda.current_stream().synchronize()
        _ARANGE_I32[dev] = cached
    return cached[:n]


def _join_probe_unique(table: JoinTable, lk: List[Column], nl: int, how: str,
                       right_matched: Optional[torch.Tensor]):
    """Single-pass probe: every left row has 0 or 1 matches."""
    s = _stream()
    rk = table.keys
    key_type = _join_inline_key_type(lk, rk)
    if key_type >= 0:
        lkey, lvalid, rkey = (lk[0].data.data_ptr(), _ptr(lk[0].validity),
                              rk[0].data.data_ptr())
        lh = ldesc = None
    else:
        lkey = lvalid = rkey = 0
        lh = _murmur3_tensor(lk, _JOIN_SEED)
        ldesc = _key_desc(lk)
    match = torch.empty(max(nl, 1), dtype=torch.int32, device="cuda")[:nl]
    every_row = how in ("left", "full")
    counts = None if every_row else torch.empty(
        ext.join_probe_num_blocks(nl), dtype=torch.int64, device="cuda")
    ext.join_probe_unique(_JOIN[how], key_type, lkey, lvalid, rkey, _ptr(lh),
                          _ptr(ldesc), table.desc.data_ptr(), len(lk),
                          table.head.data_ptr(), table.next.data_ptr(),
                          table.cap, match.data_ptr(), _ptr(right_matched),
                          _ptr(counts), nl, s)
    if every_row:
        # one output row per probe row: rmap is match, lmap the identity
        return _identity_map(nl), match, nl
    offsets, total = _exclusive_scan_i64(counts)
    lmap = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")[:total]
    rmap = torch.empty(max(total, 1), dtype=torch.int32, device="cuda")[:total] \
        if how == "inner" else None
    if total:
        ext.join_compact_unique(_JOIN[how], match.data_ptr(),
                                offsets.data_ptr(), lmap.data_ptr(),
                                _ptr(rmap), nl, s)
    return lmap, rmap, total


def join_probe(table: JoinTable, left: ColumnBatch, left_keys: List[int],
               how: str, right_matched: Optional[torch.Tensor] = None):
    s = _stream()
    nl = left.num_rows
    lk = [left.columns[i] for i in left_keys]
    if table.unique and nl:
        lmap, rmap, total = _join_probe_unique(table, lk, nl, how,
                                               right_matched)
    else:
        # general many-to-many path: count, scan, fill
        ldesc = _key_desc(lk)
        rdesc, head, nxt, cap = table.desc, table.head, table.next, table.cap
        lh = _murmur3_tensor(lk, _JOIN_SEED)
        counts = torch.empty(nl, dtype=torch.int64, device="cuda")
        ext.join_count(_JOIN[how], lh.data_ptr(), ldesc.data_ptr(),
                       rdesc.data_ptr(), len(lk), head.data_ptr(),
                       nxt.data_ptr(), cap, counts.data_ptr(), nl, s)
        offsets, total = _exclusive_scan_i64(counts)
        lmap = torch.empty(max(total, 1), dtype=torch.int32,
                           device="cuda")[:total]
        rmap = torch.empty(max(total, 1), dtype=torch.int32,
                           device="cuda")[:total] \
            if how in ("inner", "left", "full") else None
        if total:
            ext.join_fill(_JOIN[how], lh.data_ptr(), ldesc.data_ptr(),
                          rdesc.data_ptr(), len(lk), head.data_ptr(),
                          nxt.data_ptr(), cap, offsets.data_ptr(),
                          lmap.data_ptr(), _ptr(rmap), _ptr(right_matched),
                          nl, s)
    lcol = Column(DType.int32(), total, lmap, None, null_count=0)
    rcol = Column(DType.int32(), total, rmap, None, null_count=0) \
        if rmap is not None else None
    return lcol, rcol


def join_gather_maps(left: ColumnBatch, right: ColumnBatch,
                     left_keys: List[int], right_keys: List[int], how: str,
                     right_matched: Optional[torch.Tensor] = None):
    return join_probe(join_build_table(right, right_keys), left, left_keys,
                      how, right_matched)


# ---------------------------------------------------------------------------
# sort: stable LSD radix over order-preserving u64 keys (native/hipdf sort.hip)
# ---------------------------------------------------------------------------

# HipdfSortKind of native/hipdf/include/hipdf.h
_SORT_KEY_FIXED, _SORT_KEY_STRING, _SORT_KEY_DECIMAL128 = 0, 1, 2


def range_key(col: Column, desc: bool, nulls_last: bool) -> Column:
    """Monotone int64 proxy of the sort position of each row (signed order;
    ties allowed). Used by external sort to range-partition rows into
    bounded buckets before the in-core sort of each bucket."""
    n = col.size
    s = _stream()
    keys = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")[:n]
    if n:
        if col.dtype.id is TypeId.STRING:
            # first 8 bytes as the proxy (ties share a bucket)
            ext.make_sort_keys_str(col.offsets.data_ptr(),
                                   col.data.data_ptr(), _ptr(col.validity),
                                   0, desc, 0, keys.data_ptr(), n, s)
        elif col.dtype.id is TypeId.DECIMAL128:
            ext.make_sort_keys_i128(col.data.data_ptr(),
                                    _ptr(col.validity), 0, desc, 1,
                                    keys.data_ptr(), n, s)
        else:
            ext.make_sort_keys(_ht(col.dtype), col.data.data_ptr(),
                               _ptr(col.validity), 0, desc, nulls_last,
                               False, keys.data_ptr(), n, s)
    kc = Column(DType.int64(), n, keys, None, null_count=0)
    # make_sort_keys output orders UNSIGNED; bias the top bit for signed use
    kc = binary_op_scalar("bitxor", kc, -(1 << 63), DType.int64())
    if col.validity is not None:
        extreme = (1 << 63) - 1 if nulls_last else -(1 << 63)
        nm = is_null(col)
        kc = if_else(nm, Column.full(extreme, DType.int64(), n, "cuda"), kc)
    return Column(DType.int64(), n, kc.data, None, null_count=0)


def sort_order(batch: ColumnBatch, key_idx: List[int], descending: List[bool],
               nulls_last: List[bool]) -> Column:
    n = batch.num_rows
    s = _stream()
    if n == 0:
        return _empty_col(DType.int32())
    # key descriptors for the native call, most significant first:
    # (kind, htype, data, valid, offsets, desc, nulls_last, has_valid, nchunks)
    descs = []
    for ci, desc, nl in zip(key_idx, descending, nulls_last):
        col = batch.columns[ci]
        has_valid = col.validity is not None
        if col.dtype.id is TypeId.STRING:
            # LSD over 8-byte big-endian chunks: the host needs the longest
            # string to know how many chunks there are
            lens = Column(DType.int32(), n, col.offsets[1:], None,
                          null_count=0)
            starts0 = Column(DType.int32(), n, col.offsets[:n], None,
                             null_count=0)
            ldiff = _binary("sub", lens, starts0, None, DType.int32())
            maxlen = reduce("max", ldiff) or 0
            nchunks = max(1, (int(maxlen) + 7) // 8)
            descs.append((_SORT_KEY_STRING, 4, col.data.data_ptr(),
                          _ptr(col.validity), col.offsets.data_ptr(),
                          bool(desc), bool(nl), has_valid, nchunks))
        elif col.dtype.id is TypeId.DECIMAL128:
            descs.append((_SORT_KEY_DECIMAL128, 4, col.data.data_ptr(),
                          _ptr(col.validity), 0, bool(desc), bool(nl),
                          has_valid, 0))
        else:
            descs.append((_SORT_KEY_FIXED, _ht(col.dtype),
                          col.data.data_ptr(), _ptr(col.validity), 0,
                          bool(desc), bool(nl), has_valid, 0))
    ncounts = 256 * ext.sort_num_blocks(n)
    # scratch of the whole sort in two allocations: u64 keys x2, counts,
    # their scan, the scan's own scratch and the varying-bits word; i32 perms
    nscan = ext.scan_scratch_elems(ncounts)
    w64 = torch.empty(2 * n + 2 * ncounts + nscan + 1, dtype=torch.int64,
                      device="cuda")
    w32 = torch.empty(2 * n, dtype=torch.int32, device="cuda")
    perm = torch.empty(n, dtype=torch.int32, device="cuda")
    p64, p32 = w64.data_ptr(), w32.data_ptr()
    counts_p = p64 + 16 * n
    scanned_p = counts_p + 8 * ncounts
    scratch_p = scanned_p + 8 * ncounts
    ext.sort_order(descs, n, p64, p64 + 8 * n, p32, p32 + 4 * n, counts_p,
                   scanned_p, scratch_p, scratch_p + 8 * nscan,
                   perm.data_ptr(), s)
    return Column(DType.int32(), n, perm, None, null_count=0)


def str_pad(col: Column, width: int, fill: str, left: bool) -> Column:
    n = col.size
    s = _stream()
    v = col.validity.clone() if col.validity is not None else None
    fb = fill.encode("utf-8")
    fill_t = _pattern_tensor(fill) if fb else torch.zeros(
        1, dtype=torch.uint8, device="cuda")
    lens = torch.empty(max(n, 1), dtype=torch.int64, device="cuda")[:n]
    if n:
        ext.str_pad(1 if left else 0, col.offsets.data_ptr(),
                    col.data.data_ptr(), fill_t.data_ptr(), len(fb),
                    len(fill), width, 0, lens.data_ptr(), 0, 0, n, s)
    scanned, total = _exclusive_scan_i64(lens) if n else (lens, 0)
    out = torch.empty(max(total, 1), dtype=torch.uint8,
                      device="cuda")[:total]
    if total:
        ext.str_pad(1 if left else 0, col.offsets.data_ptr(),
                    col.data.data_ptr(), fill_t.data_ptr(), len(fb),
                    len(fill), width, scanned.data_ptr(), lens.data_ptr(),
                    out.data_ptr(), 1, n, s)
    offs = torch.empty(n + 1, dtype=torch.int32, device="cuda")
    if n:
        ext.narrow_i64_i32(scanned.data_ptr(), offs.data_ptr(), n, s)
    offs[n] = total
    return Column(DType.string(), n, out, v, offs,
                  null_count=col._null_count)


def str_locate(col: Column, substr: str, pos: int = 1) -> Column:
    n = col.size
    s = _stream()
    v = col.validity.clone() if col.validity is not None else None
    nb = substr.encode("utf-8")
    needle = _pattern_tensor(substr) if nb else torch.zeros(
        1, dtype=torch.uint8, device="cuda")
    out = _alloc(n, DType.int32())
    if n:
        ext.str_locate(col.offsets.data_ptr(), col.data.data_ptr(),
                       needle.data_ptr(), len(nb), pos, out.data_ptr(),
                       n, s)
    return Column(DType.int32(), n, out, v, null_count=col._null_count)


_TZ_DEV_CACHE: dict = {}


def _tz_device(zone: str):
    hit = _TZ_DEV_CACHE.get(zone)
    if hit is None:
        from ..tools import tzdb

        trans, offs = tzdb.load(zone)
        hit = (torch.from_numpy(trans.copy()).cuda(),
               torch.from_numpy(offs.copy()).cuda())
        _TZ_DEV_CACHE[zone] = hit
    return hit


def tz_convert(col: Column, zone: str, to_utc: bool) -> Column:
    n = col.size
    s = _stream()
    v = col.validity.clone() if col.validity is not None else None
    trans, offs = _tz_device(zone)
    out = _alloc(n, DType.timestamp())
    if n:
        ext.tz_convert(col.data.data_ptr(), trans.data_ptr(),
                       offs.data_ptr(), trans.numel(), 1 if to_utc else 0,
                       out.data_ptr(), n, s)
    return Column(DType.timestamp(), n, out, v,
                  null_count=col._null_count)


def _token_tensor(tokens):
    flat = []
    for kind, arg in tokens:
        flat.extend([kind, arg])
    return torch.tensor(flat, dtype=torch.int32).cuda()


def date_format(col: Column, tokens, width: int) -> Column:
    n = col.size
    s = _stream()
    v = col.validity.clone() if col.validity is not None else None
    tok = _token_tensor(tokens)
    out = torch.empty(max(n * width, 1), dtype=torch.uint8,
                      device="cuda")[:n * width]
    if n:
        ext.date_format(col.data.data_ptr(), tok.data_ptr(), len(tokens),
                        width, out.data_ptr(), n, s)
    offs = torch.arange(0, (n + 1) * width, width, dtype=torch.int32,
                        device="cuda")
    return Column(DType.string(), n, out, v, offs,
                  null_count=col._null_count)


def ts_parse(col: Column, tokens, width: int) -> Column:
    n = col.size
    s = _stream()
    tok = _token_tensor(tokens)
    out = _alloc(n, DType.timestamp())
    ov = _alloc_mask(n)
    if n:
        ext.ts_parse(col.offsets.data_ptr(), col.data.data_ptr(),
                     _ptr(col.validity), tok.data_ptr(), len(tokens),
                     width, out.data_ptr(), ov.data_ptr(), n, s)
    return Column(DType.timestamp(), n, out, ov, null_count=None)


def and_parent_validity(kid: Column, parent: Column) -> Column:
    """Null out child rows where the parent (struct) row is null."""
    if parent.validity is None:
        return kid
    n = kid.size
    s = _stream()
    mask = _and_masks(kid.validity, parent.validity) \
        if kid.validity is not None else parent.validity.clone()
    return Column(kid.dtype, n, kid.data, mask, kid.offsets,
                  null_count=None, child=kid.child)


def _xxhash64_tensor(cols: List[Column], seed: int = 42,
                     sel: Optional[torch.Tensor] = None,
                     n_out: Optional[int] = None) -> torch.Tensor:
    """Column-chained xxHash64 (Hash.xxhash64 analogue; fixed-width
    values widened to 8 bytes, floats normalized, strings over bytes)."""
    n = cols[0].size if sel is None else (n_out if n_out is not None
                                          else sel.numel())
    s = _stream()
    seeds = torch.full((max(n, 1),), seed, dtype=torch.int64,
                       device="cuda")[:n]
    selp = 0 if sel is None else sel.data_ptr()
    for c in cols:
        if n == 0:
            break
        if c.dtype.id is TypeId.STRING:
            ext.xxhash64_str(c.offsets.data_ptr(), c.data.data_ptr(),
                             _ptr(c.validity), selp, seeds.data_ptr(), n, s)
        else:
            ext.xxhash64_col(_HASH_KIND[c.dtype.id], _ht(c.dtype),
                             c.data.data_ptr(), _ptr(c.validity), selp,
                             seeds.data_ptr(), n, s)
    return seeds


def xxhash64(cols: List[Column], seed: int = 42) -> Column:
    t = _xxhash64_tensor(cols, seed)
    return Column(DType.int64(), cols[0].size, t, None, null_count=0)


# algo id of hipdf_digest_hex and the hex digits of a result
_DIGEST = {"md5": (0, 32), "sha1": (1, 40), "sha224": (2, 56),
           "sha256": (3, 64), "sha384": (4, 96), "sha512": (5, 128)}


def _need_string(fn: str, col: Column):
    if col.dtype.id is not TypeId.STRING:
        raise TypeError(f"{fn} needs a string input, got {col.dtype}")


def digest_hex(col: Column, algo: str) -> Column:
    """md5 / sha1 / sha2 of each row's UTF-8 bytes as lowercase hex: one
    launch, thread per row. Every result has the same width W, so the
    offsets are arange * W and nothing is sized or scanned."""
    _need_string(algo, col)
    aid, width = _DIGEST[algo]
    n = col.size
    if n == 0:
        return _empty_col(DType.string())
    if n * width > 2 ** 31 - 1:
        raise OverflowError(f"{algo} result exceeds int32 offsets")
    v = col.validity.clone() if col.validity is not None else None
    out = torch.empty(n * width, **_NO_DATA)
    ext.digest_hex(aid, col.offsets.data_ptr(), col.data.data_ptr(),
                   _ptr(col.validity), out.data_ptr(), n, _stream())
    offs = torch.arange(0, (n + 1) * width, width, dtype=torch.int32,
                        device="cuda")
    return Column(DType.string(), n, out, v, offs, col._null_count)


def crc32(col: Column) -> Column:
    """zlib crc32 of each row's UTF-8 bytes, unsigned, as INT64."""
    _need_string("crc32", col)
    n = col.size
    if n == 0:
        return _empty_col(DType.int64())
    v = col.validity.clone() if col.validity is not None else None
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    ext.crc32_str(col.offsets.data_ptr(), col.data.data_ptr(),
                  _ptr(col.validity), out.data_ptr(), n, _stream())
    return Column(DType.int64(), n, out, v, None, col._null_count)


def _gb_hll(vc: Column, row_gid: torch.Tensor, selp, n: int, ngroups: int,
            p: int, s) -> Column:
    import numpy as np

    sel_t = None
    if selp:
        raise NotImplementedError("approx_count_distinct under filter "
                                  "fusion")
    from .cpu_backend import _hll_estimate_host

    hashes = _xxhash64_tensor([vc], 42)
    m = 1 << p
    regs = torch.zeros(max(ngroups * m, 1), dtype=torch.uint8,
                       device="cuda")
    if n:
        ext.gb_hll(hashes.data_ptr(), _ptr(vc.validity),
                   row_gid.data_ptr(), 0, regs.data_ptr(), p, n, s)
    regs_np = regs.cpu().numpy().reshape(ngroups, m)
    est = _hll_estimate_host(regs_np)
    return Column.from_numpy(est, DType.int64()).cuda()
