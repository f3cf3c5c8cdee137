"""Runs encoder cases in a process of its own: the library reads its dispatch switches (PCV_LN32_MAX_M,
PCV_ATTN_NO_PERSIST, PCV_GEMM_WS) once per process, so tests/test_encoder_paths_gpu.py starts this script with the
switch in the environment.  TEST INFRASTRUCTURE ONLY.

    python encoder_child.py cases.npz results.npz

cases.npz: "cases", a JSON list of {desc, compute, seed}, and "ids<i>" / "mask<i>" per case.
results.npz: "out<i>" and, up to the debug token limit, "hid<i>" [(layers + 1), B, L, hidden]."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(src, dst):
    import encoder_paths as ep
    import perceive_amd as pa

    data = np.load(src)
    cases = json.loads(str(data["cases"]))
    ctx = pa.Context(0)
    res = {}
    for i, case in enumerate(cases):
        m = ep.build_model(pa, ctx, case["desc"], case["compute"], case["seed"])
        out, hid = ep.run_model(m, case, data[f"ids{i}"], data[f"mask{i}"])
        m.close()
        res[f"out{i}"] = out
        if hid is not None:
            res[f"hid{i}"] = hid
    ctx.close()
    np.savez(dst, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
