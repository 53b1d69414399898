"""Generates tests/golden/register_parent.npz: what the CPU build of the registration headers (csrc/register.h, csrc/register_icp.h,
through the g++ stubs under tests/stub/) returns for every case of tests/test_register_icp_cpu.py's frozen_cases(), frozen so
that a change to those headers that is meant to move no byte can be checked against the commit before it.

Run it on the commit whose bytes are to be kept, from the repo root:  python tests/golden/make_register_parent.py
For each case the file holds the SHA-256 of the inputs (arrays, starts, options), the result structs' bytes and, for sources of at
most FROZEN_IDX_MAX points, idx.  It reads nothing outside the repository and needs no GPU.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_align_cpu, test_register_cpu, test_register_icp_cpu as t  # noqa: E402


def stub(module, flags=()):
    so = os.path.join(tempfile.mkdtemp(prefix="register_parent_"), "stub.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *flags, "-shared", "-fPIC", "-o", so, module.STUB])
    return module.load_stub(so)


def main():
    rg, ig, al = stub(test_register_cpu), stub(t), stub(test_align_cpu, ["-pthread"])
    out, names = {}, []
    for name, entry, tgt, src, nrm, starts, kw in t.frozen_cases():
        res, idx = t.frozen_stub_run(rg, ig, al, entry, tgt, src, nrm, starts, kw)
        names.append(name)
        out[name + " | sha"] = np.array(t.frozen_hash(tgt, src, nrm, starts, kw))
        out[name + " | res"] = np.frombuffer(res, np.uint8)
        if len(src) <= t.FROZEN_IDX_MAX:
            out[name + " | idx"] = np.ascontiguousarray(idx, np.int32)
        print(f"{name}: {len(res)} result bytes, source {len(src)}")
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    np.savez_compressed(t.FROZEN, names=np.array(names), commit=np.array(commit), **out)
    print(f"{t.FROZEN}: {len(names)} cases of commit {commit or '?'}, {os.path.getsize(t.FROZEN)} bytes")


if __name__ == "__main__":
    main()
