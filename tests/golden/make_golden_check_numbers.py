"""Writes tests/golden/check_numbers.json: what ops.check_speed / check_pitch / check_loudness / check_true_peak / check_duration return or raise over one
fixed list of inputs.  It was run ONCE, at the commit before the five functions became calls of one helper, so the table is the behaviour of the five
separate copies; tests/test_host_logic.py asserts that today's functions reproduce it.  The script refuses to write from any other checkout: the table never comes from the code it checks.

    python tests/golden/make_golden_check_numbers.py

A row is [input, B, name, outcome]: the input as the Python expression that evaluates to it (`nan`, `inf` are the floats), the `name=` keyword (null: the
function's default), the outcome as repr(result) or "<exception type>: <message>".
"""
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

# function -> (lo, hi, the value that asks for nothing, or None where only None does)
RANGES = dict(check_speed=(0.5, 2.0, 1.0), check_pitch=(-12.0, 12.0, 0.0), check_loudness=(-50.0, -5.0, None), check_true_peak=(-20.0, 0.0, None),
              check_duration=(0.02, 80.0, None))
B = 3
RECORDED_AT = "dc92900"   # the last commit with five separate check_* functions: the only one this script writes the table from


def inputs(lo, hi, neutral):
    """[(expression, B)]: None, a bool, a str, NaN, inf, both range ends, just outside both, a wrong length, a None entry, a bool entry, all-neutral lists"""
    mid = 0.75 * lo + 0.25 * hi
    below, above = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
    vals = ["None", "True", "False", "'1'", "b'1'", "{}", "nan", "inf", "-inf", repr(lo), repr(hi), repr(below), repr(above), repr(mid), repr(int(hi)),
            f"[{mid!r}, {mid!r}]", f"[{mid!r}] * 4", "[]", f"({lo!r}, {hi!r}, {mid!r})", f"[{mid!r}, None, {hi!r}]", f"[None, {lo!r}, None]", f"[{mid!r}, True, {mid!r}]",
            f"[{mid!r}, '1', {mid!r}]", f"[{mid!r}, [{mid!r}], {mid!r}]", f"[{mid!r}, nan, {mid!r}]", f"[{mid!r}, {mid!r}, -inf]", f"[{lo!r}, {above!r}, {hi!r}]",
            f"[{below!r}, {mid!r}, {mid!r}]", "[None, None, None]", "(None, None, None)"]
    if neutral is not None:
        vals += [repr(neutral), repr(int(neutral)), f"[{neutral!r}] * 3", f"[{neutral!r}, None, {int(neutral)!r}]", f"[{neutral!r}, {mid!r}, None]"]
    out = [(v, B) for v in vals]
    return out + [("None", 0), ("[]", 0), (repr(mid), 1), (repr(mid), 0), (f"[{mid!r}]", 1)]


def outcome(fn, expr, b, **kw):
    try:
        return repr(fn(eval(expr, {"__builtins__": {}, "nan": math.nan, "inf": math.inf}), b, **kw))
    except (TypeError, ValueError) as e:
        return f"{type(e).__name__}: {e}"


def table(ops):
    out = {}
    for name, (lo, hi, neutral) in RANGES.items():
        fn = getattr(ops, name)
        out[name] = [[expr, b, None, outcome(fn, expr, b)] for expr, b in inputs(lo, hi, neutral)]
        out[name] += [[expr, b, "arg", outcome(fn, expr, b, name="arg")] for expr, b in (("'x'", 2), ("[1.0]", 2), (f"[{hi!r}, inf]", 2), ("[None, False]", 2))]  # name= travels
    return out


if __name__ == "__main__":
    import subprocess
    from chatterbox_amd import ops
    at = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=HERE, capture_output=True, text=True).stdout.strip()
    if hasattr(ops, "_per_request_numbers") or at != RECORDED_AT:
        sys.exit(f"refused: the table records the five separate functions of commit {RECORDED_AT}; this checkout ({at or 'no git'}) holds the code the table checks")
    with open(os.path.join(HERE, "check_numbers.json"), "w") as fh:
        fh.write("{\n" + f'"_recorded_at_commit": {json.dumps(at)},\n' + ",\n".join(f'{json.dumps(k)}: [\n' + ",\n".join(json.dumps(row) for row in rows) + "\n]" for k, rows in table(ops).items()) + "\n}\n")
