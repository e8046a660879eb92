"""CPU (-m "not gpu"): the path of the delivery options, pinned as data that was recorded before the path was folded into one record and one chain.
tests/golden/delivery_chain.json (delivery_chain_common.py): the ops calls of vocode behind the vocoder for every combination of the options, the keywords
synthesize hands to vocode, and _checked_job's reading of a job.  tests/golden/api_calls_delivery.json (api_calls_common.record_delivery): what the public classes
hand to their engines for format, loudness, pauses, pitch, word_times and guard.  Equality with both is the statement that the fold leaves the launches, their
order, the results' structure and the engine calls alone.  Nothing is launched."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def _same(path, got, label):
    import delivery_chain_common as C
    with open(path) as f:
        want = C.unpack(json.load(f))
    got = json.loads(json.dumps(got))   # (through JSON: tuples and lists compare alike)
    for k, (w, g) in enumerate(zip(want, got)):
        name = f"entry {k}: {label(w)}"
        assert label(w) == label(g), name
        assert sorted(w) == sorted(g), f"{name}: the keys differ"
        for key in w:
            assert w[key] == g[key], f"{name}: {key}"
    assert len(got) == len(want)
    return want


def test_every_step_of_the_delivery_chain_equals_the_recorded_one():
    import delivery_chain_common as C
    want = _same(C.FIXTURE, C.record(), lambda e: (e["what"], e.get("case"), e.get("on"), e.get("sync")))
    assert len(want) > 200 and {e["what"] for e in want} == {"vocode", "ChatterboxEngine.synthesize", "TurboEngine.synthesize", "_checked_job"}
    assert sum(e["what"] == "vocode" for e in want) == 2 ** 7 - 2 ** 5 + 1, "every combination of six options and sync, loudness with a join once"


def test_every_engine_call_with_delivery_options_equals_the_recorded_one():
    import api_calls_common as A
    want = _same(A.FIXTURE_DELIVERY, A.record_delivery(), lambda e: (e["scenario"], e["call"]))
    assert len(want) > 100 and {e["scenario"].split("/")[0] for e in want} == {"ChatterboxTTS", "ChatterboxMultilingualTTS", "ChatterboxTurboTTS", "ChatterboxVC"}
    jobs = [j for e in want if e["scenario"].endswith("delivery_batch") for j in e["kw"].get("jobs", [e["kw"]])]
    for option in ("loudness", "pauses", "pitch"):
        assert any(option in j for j in jobs) and any(option not in j for j in jobs), f"{option}: a sub-batch carries it only when one of its requests uses it"
    marked = [e for e in want if e["scenario"].endswith("watermarked")]
    assert marked and all("format" not in j for e in marked for j in e["kw"].get("jobs", [e["kw"]])), "with a watermarker the engine receives no format"


def test_the_option_path_has_one_copy_of_each_check():
    """what the fold was for, as counts on the source: one loudness check and one stream scope in engine.py"""
    src = open(os.path.join(os.path.dirname(HERE), "chatterbox_amd", "engine.py")).read()
    assert src.count("ops.check_loudness(") == 1
    assert src.count("if hift_stream is not None else contextlib.nullcontext()") == 1
