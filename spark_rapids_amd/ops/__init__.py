"""Columnar op dispatch: device columns -> hand-written HIP kernels (hipdf),
host columns -> CPU reference backend.

The GPU path NEVER silently falls back to eager torch/CPU compute: if the
native extension is missing on a machine with a GPU, ops raise. This is the
boundary the reference crosses via JNI into libcudf
(reference: SURVEY.md section 2.8 kernel surface).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

from ..column import Column, ColumnBatch
from ..types import DType

from . import cpu_backend

_gpu = None
_gpu_err: Optional[str] = None


def _gpu_backend():
    global _gpu, _gpu_err
    if _gpu is None and _gpu_err is None:
        try:
            from . import gpu_backend as g
            _gpu = g
        except Exception as e:  # noqa: BLE001
            _gpu_err = f"hipdf native extension unavailable: {e!r}"
    if _gpu is None:
        raise RuntimeError(_gpu_err)
    return _gpu


def backend_for(*cols: Column):
    if any(c.is_cuda for c in cols):
        return _gpu_backend()
    return cpu_backend


def binary_op(op: str, lhs: Column, rhs: Column, out_dtype: DType) -> Column:
    return backend_for(lhs, rhs).binary_op(op, lhs, rhs, out_dtype)


def binary_op_scalar(op: str, lhs: Column, scalar, out_dtype: DType) -> Column:
    return backend_for(lhs).binary_op_scalar(op, lhs, scalar, out_dtype)


def str_split(col: Column, delimiter: str) -> Column:
    return backend_for(col).str_split(col, delimiter)


def array_size(col: Column) -> Column:
    return backend_for(col).array_size(col)


def array_contains(col: Column, value) -> Column:
    """array_contains(array, value) -> bool; null array -> null
    (GpuArrayContains analogue)."""
    return backend_for(col).array_contains(col, value)


def element_at(col: Column, index: int) -> Column:
    return backend_for(col).element_at(col, index)


def sort_array(col: Column, ascending: bool = True,
               nulls_first: bool = True) -> Column:
    """Stable sort inside each list by (null rank, value); NaN greatest,
    null list -> null (GpuSortArray / GpuArraySort analogue)."""
    return backend_for(col).sort_array(col, ascending, nulls_first)


def array_distinct(col: Column) -> Column:
    """First occurrence of each value per list, input order kept
    (GpuArrayDistinct KEEP_FIRST)."""
    return backend_for(col).array_distinct(col)


def array_min(col: Column) -> Column:
    """Least non-null element per list; NULL when there is none."""
    return backend_for(col).array_min(col)


def array_max(col: Column) -> Column:
    return backend_for(col).array_max(col)


def array_union(a: Column, b: Column) -> Column:
    """Distinct elements of a, then those of b not in a, first-occurrence
    order; NULL when either row is (GpuArrayUnion analogue)."""
    return backend_for(a, b).array_union(a, b)


def array_intersect(a: Column, b: Column) -> Column:
    """Distinct elements of a that occur in b, a's order (GpuArrayIntersect)."""
    return backend_for(a, b).array_intersect(a, b)


def array_except(a: Column, b: Column) -> Column:
    """Distinct elements of a that do not occur in b (GpuArrayExcept)."""
    return backend_for(a, b).array_except(a, b)


def arrays_overlap(a: Column, b: Column) -> Column:
    """True on a shared non-null element, else NULL when both are non-empty
    and either holds a null, else false (GpuArraysOverlap)."""
    return backend_for(a, b).arrays_overlap(a, b)


def array_position(col: Column, needle: Column) -> Column:
    """INT64 1-based place of the first element equal to the row's entry of
    `needle` (a column of the element type), 0 when there is none; NULL
    when the row or the needle is. Equality is array_distinct's, and a null
    element equals nothing (GpuArrayPosition analogue)."""
    return backend_for(col, needle).array_position(col, needle)


def array_remove(col: Column, needle: Column) -> Column:
    """The array without every element equal to the row's needle; order,
    null elements and bit patterns are kept; NULL when the row or the
    needle is (GpuArrayRemove analogue)."""
    return backend_for(col, needle).array_remove(col, needle)


def array_slice(col: Column, start: Column, length: Column) -> Column:
    """slice(array, start, length) with INT32 start and length columns:
    1-based start, negative from the end, an empty array when it falls
    outside the row; NULL when any of the three is. start == 0 or
    length < 0 in a row where none is null raises ValueError with Spark's
    text (GpuSlice analogue)."""
    return backend_for(col, start, length).array_slice(col, start, length)


def array_repeat(elem: Column, count: Column) -> Column:
    """LIST of `count` (INT32) copies of the row's element: empty for
    count <= 0, NULL for a null count, nulls for a null element
    (GpuArrayRepeat analogue)."""
    return backend_for(elem, count).array_repeat(elem, count)


def create_array(cols: Sequence[Column]) -> Column:
    """array(c1, ..., ck): row i is [c1[i], ..., ck[i]]; the row is never
    NULL, an element is null where its operand is. The operands have one
    type and one size (GpuCreateArray analogue)."""
    return backend_for(*cols).create_array(list(cols))


def array_concat(cols: Sequence[Column]) -> Column:
    """concat(a1, ..., ak) over LIST columns of one type: the rows'
    elements in operand order, null elements kept; NULL when any operand
    row is (GpuConcat analogue)."""
    return backend_for(*cols).array_concat(list(cols))


def array_flatten(col: Column) -> Column:
    """flatten(LIST<LIST<T>>): the row's inner arrays concatenated; NULL
    when the row or any inner array of it is (GpuFlatten analogue)."""
    return backend_for(col).array_flatten(col)


def sequence(start: Column, stop: Column,
             step: Optional[Column] = None) -> Column:
    """sequence(start, stop[, step]) over INT32 or INT64 columns of one
    type; step None is 1 where start <= stop, else -1. NULL when any
    operand is; a zero step or one pointing away from stop (with start !=
    stop) raises ValueError for the first such row; a result over
    2**31 - 1 elements raises OverflowError (GpuSequence analogue)."""
    cols = [c for c in (start, stop, step) if c is not None]
    return backend_for(*cols).sequence(start, stop, step)


def array_join(col: Column, delimiter: str,
               null_replacement: Optional[str] = None) -> Column:
    """array_join(LIST<STRING>, delimiter[, replacement]): the non-null
    elements joined by the delimiter, null ones skipped or replaced; NULL
    when the array is (GpuArrayJoin analogue)."""
    return backend_for(col).array_join(col, delimiter, null_replacement)


def list_span(col: Column) -> Tuple[int, int]:
    """(offsets[0], offsets[n] - offsets[0]) of a LIST column: where its
    elements start in the child and how many there are. The one host read
    of the higher-order functions; pass it on as `span` to spare the ops
    below their own."""
    return backend_for(col).list_span(col)


def list_element_rows(col: Column, with_pos: bool = True,
                      span: Optional[Tuple[int, int]] = None):
    """(rowid, pos): two int32 columns with one row per element of the LIST
    column from offsets[0] — the row that owns the element and its 0-based
    position in that row (None when with_pos is false). rowid gathers outer
    columns down to the elements for a lambda body."""
    return backend_for(col).list_element_rows(col, with_pos, span)


def array_filter(col: Column, pred: Column,
                 span: Optional[Tuple[int, int]] = None) -> Column:
    """filter(array, x -> pred): `pred` is a BOOL column with one row per
    element from offsets[0]; elements whose predicate is false or NULL
    drop, order kept, null rows stay null (GpuArrayFilter analogue)."""
    return backend_for(col, pred).array_filter(col, pred, span)


def array_exists(col: Column, pred: Column,
                 span: Optional[Tuple[int, int]] = None) -> Column:
    """exists(array, x -> pred), three-valued: true if any predicate is
    true, else NULL if any is NULL, else false (GpuArrayExists analogue)."""
    return backend_for(col, pred).array_exists(col, pred, span)


def array_forall(col: Column, pred: Column,
                 span: Optional[Tuple[int, int]] = None) -> Column:
    """forall(array, x -> pred): false if any predicate is false, else NULL
    if any is NULL, else true."""
    return backend_for(col, pred).array_forall(col, pred, span)


def map_keys(col: Column) -> Column:
    """MAP -> LIST<key>: shares the offsets and the entry key child
    buffer (zero-copy, reference GpuMapKeys)."""
    return Column(DType.list_(col.dtype.children[0]), col.size, col.data,
                  col.validity, col.offsets, col._null_count,
                  col.child.child[0])


def map_values(col: Column) -> Column:
    return Column(DType.list_(col.dtype.children[1]), col.size, col.data,
                  col.validity, col.offsets, col._null_count,
                  col.child.child[1])


def map_entries(col: Column) -> Column:
    """MAP -> LIST<STRUCT<key,value>> (zero-copy view of the entries)."""
    return Column(DType.list_(col.dtype.entry_dtype), col.size, col.data,
                  col.validity, col.offsets, col._null_count, col.child)


def map_get(col: Column, key) -> Column:
    """element_at(map, key): the value for `key` per row, NULL when the
    key is absent or the map is null (GpuElementAt over maps)."""
    return backend_for(col).map_get(col, key)


def make_map(kcols: Sequence[Column], vcols: Sequence[Column]) -> Column:
    """create_map(k1,v1,k2,v2,...): one map per row with a fixed entry
    list; entries keep source order (no dedup; lookups are LAST_WIN —
    map_get returns the last match, matching dict() view semantics)."""
    return backend_for(*kcols, *vcols).make_map(list(kcols), list(vcols))


def regexp_extract(col: Column, pattern: str, group: int) -> Column:
    return backend_for(col).regexp_extract(col, pattern, group)


def concat_ws(sep: str, cols: Sequence[Column]) -> Column:
    return backend_for(*cols).concat_ws(sep, list(cols))


def get_json_object(col: Column, path: str) -> Column:
    return backend_for(col).get_json_object(col, path)


def get_json_object_multi(col: Column, steps_list) -> List[Column]:
    """Several paths over one column, each given as parsed steps
    (expr/json_path.py; None for a malformed path): one column per entry."""
    return backend_for(col).get_json_object_multi(col, list(steps_list))


def regexp_extract_all(col: Column, pattern: str, group: int) -> Column:
    return backend_for(col).regexp_extract_all(col, pattern, group)


def regexp_replace(col: Column, pattern: str, replacement: str) -> Column:
    return backend_for(col).regexp_replace(col, pattern, replacement)


def decimal_mul_div(op: str, lhs: Column, rhs: Column,
                    out_dtype: DType) -> Column:
    """Exact decimal multiply/divide at the Spark result scale (operands
    keep their own scales; reference analogue: GpuMultiply/GpuDivide over
    cudf fixed-point with Spark's DecimalPrecision typing)."""
    return backend_for(lhs, rhs).decimal_mul_div(op, lhs, rhs, out_dtype)


def unary_op(op: str, col: Column, out_dtype: Optional[DType] = None) -> Column:
    return backend_for(col).unary_op(op, col, out_dtype or col.dtype)


def cast(col: Column, to: DType) -> Column:
    if col.dtype == to:
        return col
    return backend_for(col).cast(col, to)


def is_null(col: Column) -> Column:
    return backend_for(col).is_null(col)


def apply_boolean_mask(batch: ColumnBatch, mask: Column) -> ColumnBatch:
    """Filter: keep rows where mask is true (null mask = drop)."""
    return backend_for(*batch.columns, mask).apply_boolean_mask(batch, mask)


def gather(batch: ColumnBatch, indices: Column, check_bounds: bool = False,
           negatives: bool = True, dict_strings: bool = False) -> ColumnBatch:
    """Take rows by int32 index column; negative index -> null row
    (OutOfBoundsPolicy.NULLIFY analogue for join gather maps).
    negatives=False: the caller guarantees no -1 indices (inner/cross
    maps), so non-null source columns stay mask-free — otherwise a
    validity mask re-materializes on every gathered column and defeats
    the downstream non-null fast paths.
    dict_strings=True (a hash join's build side, GPU backend only): STRING
    columns come back as dictionary views over `indices` (DictColumn)."""
    backend = backend_for(*batch.columns, indices)
    if dict_strings and backend is not cpu_backend:
        return backend.gather_dict(batch, indices, negatives)
    return backend.gather(batch, indices, check_bounds, negatives)


def murmur3_hash(cols: Sequence[Column], seed: int = 42) -> Column:
    """Spark-compatible murmur3_x86_32 row hash over the columns."""
    return backend_for(*cols).murmur3_hash(list(cols), seed)


def xxhash64(cols: Sequence[Column], seed: int = 42) -> Column:
    """Canonical XXH64 row hash over the columns, seeds chained, INT64
    (Hash.xxhash64 / GpuXxHash64 analogue)."""
    return backend_for(*cols).xxhash64(list(cols), seed)


def digest_hex(col: Column, algo: str) -> Column:
    """md5 / sha1 / sha224 / sha256 / sha384 / sha512 of a STRING column's
    UTF-8 bytes as lowercase hex strings of one width; NULL where the input
    is (GpuMd5, GpuSha1, GpuSha2 analogue)."""
    return backend_for(col).digest_hex(col, algo)


def crc32(col: Column) -> Column:
    """crc32 (zlib polynomial) of a STRING column's UTF-8 bytes as the
    unsigned value in INT64; NULL where the input is (GpuCrc32
    analogue)."""
    return backend_for(col).crc32(col)


def hash_partition(batch: ColumnBatch, key_idx: Sequence[int], num_parts: int) -> Tuple[ColumnBatch, List[int]]:
    """Reorder rows so rows of one partition are contiguous; returns the
    reordered batch plus partition start offsets (len num_parts+1)."""
    return backend_for(*batch.columns).hash_partition(batch, list(key_idx), num_parts)


def reduce(op: str, col: Column):
    """Whole-column reduction -> python scalar or None."""
    return backend_for(col).reduce(op, col)


def group_by_aggregate(batch: ColumnBatch, key_idx: Sequence[int],
                       aggs: Sequence[Tuple[str, int, DType]]) -> ColumnBatch:
    """Hash group-by. aggs = [(op, value_col_idx, out_dtype)].
    Returns batch [keys..., agg results...]."""
    return backend_for(*batch.columns).group_by_aggregate(batch, list(key_idx), list(aggs))


def sort_order(batch: ColumnBatch, key_idx: Sequence[int],
               descending: Sequence[bool], nulls_last: Sequence[bool]) -> Column:
    """Return int32 permutation that sorts the batch by the keys."""
    return backend_for(*batch.columns).sort_order(batch, list(key_idx), list(descending), list(nulls_last))


def join_gather_maps(left: ColumnBatch, right: ColumnBatch,
                     left_keys: Sequence[int], right_keys: Sequence[int],
                     how: str, right_matched=None) -> Tuple[Column, Optional[Column]]:
    """Equi-join gather maps (left_map, right_map). For semi/anti only
    left_map is returned; full outer also records matched build rows into
    right_matched."""
    return backend_for(*left.columns, *right.columns).join_gather_maps(
        left, right, list(left_keys), list(right_keys), how, right_matched)


def join_build_table(right: ColumnBatch, right_keys: Sequence[int]):
    """Build the join table over the build side once; probe it with
    join_probe for every left batch. The table belongs to the backend that
    built it (device build side -> device probes)."""
    return backend_for(*right.columns).join_build_table(
        right, list(right_keys))


def join_probe(table, left: ColumnBatch, left_keys: Sequence[int], how: str,
               right_matched=None) -> Tuple[Column, Optional[Column]]:
    """Gather maps of `left` against a table from join_build_table; same
    return contract as join_gather_maps."""
    backend = cpu_backend if isinstance(table, tuple) else _gpu_backend()
    return backend.join_probe(table, left, list(left_keys), how,
                              right_matched)


def concat_batches(batches: Sequence[ColumnBatch]) -> ColumnBatch:
    assert batches
    return backend_for(*batches[0].columns).concat_batches(list(batches))


def str_pad(col: Column, width: int, fill: str, left: bool) -> Column:
    return backend_for(col).str_pad(col, width, fill, left)


def str_locate(col: Column, substr: str, pos: int = 1) -> Column:
    return backend_for(col).str_locate(col, substr, pos)


def tz_convert(col: Column, zone: str, to_utc: bool) -> Column:
    return backend_for(col).tz_convert(col, zone, to_utc)


def date_format(col: Column, tokens, width: int) -> Column:
    return backend_for(col).date_format(col, tokens, width)


def ts_parse(col: Column, tokens, width: int) -> Column:
    return backend_for(col).ts_parse(col, tokens, width)
