"""CPU (-m "not gpu"): every engine call the public classes make, argument for argument and in order, equals the recorded list tests/golden/api_calls.json
(api_calls_common.py: the scenarios, the recording engines and the JSON form).  The list was recorded before the host code of the request path was folded into one
copy per concern, so this is the statement that such a change leaves what reaches the engines alone."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)


def test_every_engine_call_of_the_public_classes_equals_the_recorded_one():
    import api_calls_common as C
    with open(C.FIXTURE) as f:
        want = json.load(f)
    got = json.loads(json.dumps(C.record()))   # (through JSON: tuples and lists compare alike)
    assert len(want) > 100 and {e["call"] for e in want} == {"synthesize", "synthesize_pipelined", "synthesize_stream", "vocode", "vocode_stream", "prepare_conditionals"}
    for k, (w, g) in enumerate(zip(want, got)):
        assert (w["scenario"], w["call"]) == (g["scenario"], g["call"]), f"call {k}"
        assert sorted(w["kw"]) == sorted(g["kw"]), f"call {k}: {w['scenario']} {w['call']}: the keywords differ"
        for name in w["kw"]:
            assert w["kw"][name] == g["kw"][name], f"call {k}: {w['scenario']} {w['call']}({name}=)"
    assert len(got) == len(want)
