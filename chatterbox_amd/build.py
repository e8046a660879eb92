"""Build libcbx_hip.so (in-tree) with hipcc for gfx950.  No torch / pybind dependency: a pure C-ABI library.

    python -m chatterbox_amd.build [--force]
"""
import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libcbx_hip.so")
STAMP = os.path.join(HERE, "csrc", ".build_stamp")
# -ffp-contract=on: a*b + c is fused where the SOURCE writes it as one expression and nowhere else (hipcc's default, `fast`, lets the
# backend fuse -- or SLP-vectorise into v_pk_mul + adds -- per site, so two instantiations of one template could round the same expression
# differently: the round-3 "bit-identical" decode-attention variants differed from the plain kernel by an ulp on the MI355X for that reason).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-ffp-contract=on"]


def _sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _headers():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h"))


def _digest():
    h = hashlib.sha256()
    for f in _sources() + _headers() + [os.path.join(HERE, "..", "include", "cbx.h")]:
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (need ROCm's hipcc to build libcbx_hip.so for gfx950)")


def build(force=False, verbose=True):
    dig = _digest()
    if not force and os.path.exists(LIB) and os.path.exists(STAMP) and open(STAMP).read().strip() == dig:
        return LIB
    cc = hipcc()
    objs = []
    procs = []
    os.makedirs(os.path.join(HERE, "build"), exist_ok=True)
    for src in _sources():
        obj = os.path.join(HERE, "build", os.path.basename(src) + ".o")
        objs.append(obj)
        cmd = [cc, *FLAGS, "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    fail = False
    for src, pr in procs:
        out, _ = pr.communicate()
        if pr.returncode != 0:
            fail = True
            sys.stderr.write(f"--- {src} failed:\n{out.decode()}\n")
        elif verbose and out.strip():
            print(out.decode())
    if fail:
        raise RuntimeError("hipcc failed")
    cmd = [cc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", LIB]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    with open(STAMP, "w") as f:
        f.write(dig)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
