"""Runs tools/ubench/store_sustained.hip on the GPU box (perf exploration; see the .hip header): TB/s of the pipelined
kernel's store streams for every tile order x Jacobian policy x constant-stream policy, and of a linear fill of the same bytes,
each the median over SAMPLES timed regions of PER launches.  The layout (strides, block sizes) is the real engine's for the
metric problem, 64 iterates per launch, 16 output buffers cycled.

    python tools/ubench/store_sustained.py [out.json]      (default: profiles/store_sustained.json)
"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

here = os.path.dirname(os.path.abspath(__file__))
root = os.path.dirname(os.path.dirname(here))
sys.path.insert(0, root)
so, src = os.path.join(here, "libstore_sustained.so"), os.path.join(here, "store_sustained.hip")
if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-shared", "-fPIC", "-o", so, src])


class Layout(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("P", "N", "tiles_per_phase", "NX", "NO", "NB", "off_nnz", "nnz_nl", "nnz_lin")] + \
               [("sg", C.c_longlong), ("sv", C.c_longlong), ("n_inst", C.c_int)]


ORDERS = {0: "a: one instance per XCD and round (xcd_place, today)", 1: "b: round-robin",
          2: "c: one phase of four instances per XCD and round", 3: "d: two instances per XCD pair, alternate workgroups",
          4: "e: two instances per XCD pair, alternate tiles"}
POLICY = {0: "plain", 1: "nt", 2: "sc1", 3: "sc1 nt"}


def main():
    import torch
    from lpopc_amd import problems
    from lpopc_amd.engine import NLPEngine

    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "profiles", "store_sustained.json")
    L = C.CDLL(so)
    L.ss_bytes.restype = C.c_double
    L.ss_bytes.argtypes = [C.POINTER(Layout)]
    L.ss_run.argtypes = [C.POINTER(Layout), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                         C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    B, NBUF, PER, SAMPLES = 64, 16, 4, 24
    intervals, nodes, P, NX, NU, NC = 64, 16, 4, 7, 3, 1
    eng = NLPEngine(problems.launch(intervals, nodes), n_instances=B, device=0)
    eng.set_option("instance_align", 16)
    sg, sv = eng.get_option("stride_g"), eng.get_option("stride_values")
    N, NO, NB = intervals * nodes, NX + NC, NX + NU + 2
    off_nnz = intervals * nodes * nodes        # a node's row of D without its diagonal entry: `nodes` entries
    nnz_nl = P * NO * NB * N
    nnz_lin = eng.nnz_jac - nnz_nl - P * NX * off_nnz
    assert nnz_lin >= 0 and eng.nnz_jac <= sv and P * NO * N <= sg, (eng.nnz_jac, sv, nnz_lin, sg)
    Y = Layout(P, N, N // 64, NX, NO, NB, off_nnz, nnz_nl, nnz_lin, sg, sv, B)
    nbytes = L.ss_bytes(C.byref(Y))
    assert nbytes <= 8 * B * (sv + sg)          # the linear reference fills one values buffer with all of a launch's bytes
    gs = [torch.empty(B * sg, dtype=torch.float64, device="cuda") for _ in range(NBUF)]
    vs = [torch.empty(B * (sv + sg) + 64, dtype=torch.float64, device="cuda") for _ in range(NBUF)]
    torch.cuda.synchronize()
    gp = (C.c_void_p * NBUF)(*[b.data_ptr() for b in gs])
    vp = (C.c_void_p * NBUF)(*[b.data_ptr() for b in vs])
    grid = torch.cuda.get_device_properties(0).multi_processor_count

    def run(order, jp, cp):
        us = (C.c_float * SAMPLES)()
        rc = L.ss_run(C.byref(Y), order, jp, cp, grid, gp, vp, NBUF, PER, SAMPLES, us)
        if rc:
            raise SystemExit("ss_run(%d, %d, %d) failed: %d" % (order, jp, cp, rc))
        med = statistics.median(us)
        return {"us": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2), "TBps": round(nbytes / med / 1e6, 3)}

    res = {"bytes_per_launch": nbytes, "workgroups": grid, "launches_per_sample": PER, "samples": SAMPLES, "buffers": NBUF,
           "stride_values": sv, "stride_g": sg, "rows": []}
    lin = [run(-1, 0, 0) for _ in range(3)]
    res["linear_16B_plain"] = lin
    print("linear 16 B plain: " + ", ".join("%.2f us %.3f TB/s" % (r["us"], r["TBps"]) for r in lin), flush=True)
    for order in sorted(ORDERS):
        for jp in (0, 1, 2):
            for cp in (1, 0, 3):
                r = run(order, jp, cp)
                r.update({"order": order, "order_name": ORDERS[order], "jacobian": POLICY[jp], "constant": POLICY[cp]})
                res["rows"].append(r)
                print("order %d  jac %-6s const %-6s %8.2f us (%.2f-%.2f)  %.3f TB/s" %
                      (order, POLICY[jp], POLICY[cp], r["us"], r["us_min"], r["us_max"], r["TBps"]), flush=True)
    res["linear_16B_plain_after"] = run(-1, 0, 0)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out_path)


if __name__ == "__main__":
    main()
