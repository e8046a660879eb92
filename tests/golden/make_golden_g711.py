"""Writes tests/golden/g711_tables.npz: the G.711 mu-law and A-law code of every int16 sample, as CPython's `audioop` gives them (lin2ulaw / lin2alaw at width 2;
the module left the standard library with Python 3.13, so the tests read this table instead).  Entry s + 32768 of `mulaw` / `alaw` is the code of sample s.
No reference arithmetic is involved: the provenance key names the Python that generated the file.

    python tests/golden/make_golden_g711.py
"""
import json
import os
import platform
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from provenance import provenance  # noqa: E402

if __name__ == "__main__":
    import audioop
    pcm = np.arange(-32768, 32768, dtype=np.int32).astype("<i2").tobytes()
    mulaw = np.frombuffer(audioop.lin2ulaw(pcm, 2), np.uint8)
    alaw = np.frombuffer(audioop.lin2alaw(pcm, 2), np.uint8)
    assert mulaw.shape == alaw.shape == (65536,)
    p = json.loads(str(provenance("tests/golden/make_golden_g711.py")))
    p["note"] = f"audioop.lin2ulaw / lin2alaw (width 2) of CPython {platform.python_version()} over every int16 sample; no model arithmetic"
    out = os.path.join(HERE, "g711_tables.npz")
    np.savez_compressed(out, mulaw=mulaw, alaw=alaw, provenance=np.array(json.dumps(p)))
    print(out, os.path.getsize(out), "bytes")
