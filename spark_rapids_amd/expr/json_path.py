"""The JSON path of get_json_object, parsed once for every layer: the
expression, both backends, the tagger and the SQL function.

Grammar: ``$`` followed by any number of steps

    .name       one or more characters, none of ``.`` or ``[``
    ['name']    any characters except ``'``; may be empty
    [n]         decimal digits, 0-based

A path without brackets keeps its earlier meaning: the keys between the
dots, empty segments dropped (``$``, ``$.k``, ``$.a.b``). Wildcards are not
supported and raise; any other malformed path parses to None, for which the
expression yields NULL on every row, as Spark does.
"""
from __future__ import annotations

from typing import List, Optional, Tuple, Union

KEY = 0
INDEX = 1

Step = Tuple[int, Union[str, int]]

# paths longer than this run on the CPU (the tagger's bound)
MAX_DEVICE_STEPS = 16
# paths over one column that one device parse answers (kMaxFusedPaths in
# native/hipdf/kernels/json_path.h); larger groups run in chunks
MAX_FUSED_PATHS = 8


def parse(path: str) -> Optional[List[Step]]:
    """[(KEY, name) | (INDEX, n), ...], or None for a malformed path."""
    if not path.startswith("$"):
        return None
    if "[" not in path and "]" not in path:
        keys = [k for k in path[1:].lstrip(".").split(".") if k]
        if "*" in keys:
            raise NotImplementedError("json path wildcard")
        return [(KEY, k) for k in keys]
    steps: List[Step] = []
    i, n = 1, len(path)
    while i < n:
        c = path[i]
        if c == ".":
            j = i + 1
            while j < n and path[j] not in ".[":
                j += 1
            name = path[i + 1:j]
            if not name:
                return None
            if name == "*":
                raise NotImplementedError("json path wildcard")
            steps.append((KEY, name))
            i = j
        elif c == "[":
            if path.startswith("'", i + 1):
                q = path.find("'", i + 2)
                if q < 0 or not path.startswith("]", q + 1):
                    return None
                steps.append((KEY, path[i + 2:q]))
                i = q + 2
                continue
            j = path.find("]", i)
            if j < 0:
                return None
            body = path[i + 1:j]
            if body == "*":
                raise NotImplementedError("json path wildcard")
            if body.isascii() and body.isdigit():
                steps.append((INDEX, int(body)))
            else:
                return None
            i = j + 1
        else:
            return None
    return steps


def encode(steps: List[Step]) -> Tuple[List[int], bytes]:
    """The native form: int32 triples [kind, a, b] per step, flattened, and
    the blob of key names. A key step's name is names[a:a+b]; an index
    step's index is a."""
    flat: List[int] = []
    names = bytearray()
    for kind, arg in steps:
        if kind == KEY:
            raw = arg.encode("utf-8")
            flat.extend([KEY, len(names), len(raw)])
            names.extend(raw)
        else:
            # no row holds 2^31 elements: a larger index matches nothing
            flat.extend([INDEX, min(arg, 2 ** 31 - 1), 0])
    return flat, bytes(names)
