"""Facts about the reference tree that the CPU tests compare against, stored as data so that the tests run anywhere (no reference tree needed):

  * punc_norm: the reference's `punc_norm` of mtl_tts.py / tts.py / tts_turbo.py applied to the cases of
    tests/test_host_logic.py::test_punc_norm_matches_reference (inputs and outputs only),
  * examples: what each reference example program imports from `chatterbox.*` and which methods / keyword names it calls on those classes
    (tests/test_host_logic.py::_example_api_calls; no program text),
  * py_line_counts: the line count of every .py file of the reference, by path relative to its root
    (tests/test_host_logic.py::test_reference_citations_point_into_existing_files).

    python tests/golden/make_golden_reference_meta.py      (where the reference tree is present; CBX_REFERENCE_ROOT overrides its location)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_import  # noqa: E402

OUT = os.path.join(HERE, "reference_meta.json")
PUNC_NORM_CASES = ["hello world...  how are you; fine — ok", "Déjà vu: “quoted” ‘text’ ", "x", "already done!", "multi\n line\ttext - dash",
                   "你好。", "こんにちは、", "ends with cjk comma，", ""]
EXAMPLES = ["example_tts.py", "example_tts_turbo.py", "example_tts_nano.py", "example_vc.py"]


def main():
    assert ref_import.available(), f"reference tree not found under {ref_import.REF_ROOT}"
    from test_host_logic import _example_api_calls
    punc = {}
    for fname in ("mtl_tts.py", "tts.py", "tts_turbo.py"):
        src = open(os.path.join(ref_import.REF_SRC, fname), encoding="utf-8").read()
        start = src.index("def punc_norm")
        ns = {}
        exec(src[start:src.index("@dataclass", start)], ns)
        punc[fname] = [[t, ns["punc_norm"](t)] for t in PUNC_NORM_CASES]
    examples = {}
    for name in EXAMPLES:
        imports, calls = _example_api_calls(open(os.path.join(ref_import.REF_ROOT, name), encoding="utf-8").read())
        examples[name] = {"imports": imports, "calls": [[c, m, list(k)] for c, m, k in calls]}
    counts = {}
    for root, _, files in os.walk(ref_import.REF_ROOT):
        for f in files:
            if f.endswith(".py"):
                p = os.path.join(root, f)
                with open(p, "rb") as fh:
                    counts[os.path.relpath(p, ref_import.REF_ROOT)] = sum(1 for _ in fh)
    with open(OUT, "w", encoding="utf-8") as fh:
        json.dump({"punc_norm": punc, "examples": examples, "py_line_counts": dict(sorted(counts.items()))}, fh, ensure_ascii=False, indent=1)
        fh.write("\n")
    print(OUT)


if __name__ == "__main__":
    main()
