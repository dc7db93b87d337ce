"""Exact reference for the decimal kernels, in Python ints only.

Every function works on unscaled integers (value = unscaled / 10**scale)
and returns None for NULL. Nothing here imports the engine: this is the
oracle that both backends are compared with.
"""

I128_MASK = (1 << 128) - 1
I64_MAX = (1 << 63) - 1


def half_up_div(num: int, den: int) -> int:
    """num / den rounded to the nearest integer, ties away from zero."""
    if den == 0:
        raise ZeroDivisionError("half_up_div by zero")
    sign = -1 if (num < 0) != (den < 0) else 1
    num, den = abs(num), abs(den)
    q, r = divmod(num, den)
    if 2 * r >= den:
        q += 1
    return sign * q


def _bounded(r: int, out_prec: int, out_is_64: bool = False):
    if abs(r) >= 10 ** out_prec:
        return None
    if out_is_64 and abs(r) > I64_MAX:
        return None
    return r


def mul_ref(x, y, s1, s2, out_scale, out_prec):
    """x*y at out_scale, HALF_UP, NULL past out_prec digits."""
    if x is None or y is None:
        return None
    shift = s1 + s2 - out_scale
    assert shift >= 0, "a product is never scaled up"
    r = x * y
    if shift:
        r = half_up_div(r, 10 ** shift)
    return _bounded(r, out_prec)


def div_ref(x, y, s1, s2, out_scale, out_prec):
    """x/y at out_scale, HALF_UP, NULL on y == 0 and past out_prec digits."""
    if x is None or y is None or y == 0:
        return None
    shift = out_scale + s2 - s1
    if shift >= 0:
        r = half_up_div(x * 10 ** shift, y)
    else:
        r = half_up_div(x, y * 10 ** -shift)
    return _bounded(r, out_prec)


def rescale_ref(v, shift, out_prec, out_is_64):
    """v * 10**shift (HALF_UP when shift < 0); NULL past out_prec digits or,
    for a 64-bit result, past int64."""
    if v is None:
        return None
    r = v * 10 ** shift if shift >= 0 else half_up_div(v, 10 ** -shift)
    return _bounded(r, out_prec, out_is_64)


def _both(fn):
    def wrapped(x, y):
        return None if x is None or y is None else fn(x, y)
    wrapped.__name__ = fn.__name__
    return wrapped


ARITH = {
    "add": _both(lambda x, y: x + y),
    "sub": _both(lambda x, y: x - y),
    "min": _both(lambda x, y: x if x <= y else y),
    "max": _both(lambda x, y: x if x >= y else y),
}
COMPARE = {
    "eq": _both(lambda x, y: x == y),
    "ne": _both(lambda x, y: x != y),
    "lt": _both(lambda x, y: x < y),
    "le": _both(lambda x, y: x <= y),
    "gt": _both(lambda x, y: x > y),
    "ge": _both(lambda x, y: x >= y),
}


def wrap_i128(v):
    """Two's-complement wrap to a signed 128-bit value."""
    if v is None:
        return None
    v &= I128_MASK
    return v - (1 << 128) if v >> 127 else v


def grouped_sum(keys, values, sel=None):
    """{key: (total or None, count)} over the rows in `sel` (all rows when
    None). A group whose selected values are all NULL has (None, 0)."""
    rows = range(len(keys)) if sel is None else sel
    out = {}
    for i in rows:
        total, cnt = out.get(keys[i], (None, 0))
        v = values[i]
        if v is not None:
            total = v if total is None else total + v
            cnt += 1
        out[keys[i]] = (total, cnt)
    return out
