"""Record tests/golden/fwd_launch_census.json: what each request of tests/fwd_launch_cases.py really dispatches.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o census -- python tools/record_fwd_launch_census.py run
    python tools/record_fwd_launch_census.py parse DIR/**/census_kernel_trace.csv tests/golden/fwd_launch_census.json

`run` issues every request once (random heat-maps and camera rigs: the launch does not depend on the data) with one
sp3d_debug_stamp dispatch in front of each; `parse` walks the trace in dispatch order, starts a new request at every
stamp_kernel and keeps the unproject_* dispatches: name without namespace and parameter list, workgroups, workgroup size,
LDS bytes as the trace reports them (static + dynamic).  The kernel trace runs alone - no counters, no other tracing.
The table is a record of the library it was run against: tests/test_fwd_launch_plan.py holds later libraries to it.
(The table committed with the launch plan was taken from the previous library on the host, by interposing hipLaunchKernel;
a trace recorded with this script has the same format and should equal it.)"""
import csv
import json
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests.fwd_launch_cases import requests  # noqa: E402


def run():
    import torch
    from selfpose3d_amd import _lib, synthetic as syn
    from selfpose3d_amd.camera_pack import pack_cameras
    dev = torch.device("cuda:0")
    lib = _lib.load()
    slot = torch.zeros(1, dtype=torch.int64, device=dev)
    img = (96, 72)
    for r in requests():
        B, V, J, jp, h, w = r["B"], r["V"], r["J"], r["jp"], r["h"], r["w"]
        X, Y, Z = r["cube"]
        in_dt = torch.bfloat16 if r.get("in_bf16") else torch.float32
        out_dt = torch.bfloat16 if r.get("out_bf16") else torch.float32
        cam = torch.from_numpy(pack_cameras(syn.random_meta(B, V, img, seed=B * 100 + V), B, img)).to(dev)
        centers = torch.tensor([syn.SPACE_CENTER] * B, dtype=torch.float32, device=dev)
        valid = torch.ones(B, dtype=torch.uint8, device=dev)
        nhwc = r["layout"] == "nhwc"
        if r.get("one"):
            whole = torch.rand((V, B, h, w, jp) if nhwc else (V, B, jp, h, w), device=dev)
            views = [whole[c, ..., 2] if nhwc else whole[c, :, 2] for c in range(V)]
        elif nhwc:
            views = list(torch.rand((V, B, h, w, jp), device=dev).to(in_dt))
        else:
            views = list(torch.rand((V, B, J, h, w), device=dev))
        layout = _lib.LAYOUT_NHWC if nhwc else _lib.LAYOUT_PLANAR
        kw = dict(channels_last=bool(r.get("cl")), out_dtype=out_dt, one_channel=bool(r.get("one")))
        if r["entry"] == "strided":
            px, py, pz = r.get("pad", (0, 0, 0))
            buf = torch.zeros((B, J, X + px, Y + py, Z + pz), dtype=out_dt, device=dev)
            kw.update(out=buf[:, :, :X, :Y, :Z], want_grids=False)
        elif r["entry"] == "train":
            kw["pass_mask"] = torch.zeros((B, X * Y * Z), dtype=torch.int16, device=dev)
        elif r["entry"] == "variant":
            kw["variant"] = r["word"]
        torch.cuda.synchronize()
        _lib.check(lib.sp3d_debug_stamp(slot.data_ptr(), _lib._stream(dev)), "stamp")
        if r["entry"] == "zdft":
            _lib.unproject_fwd_zdft(views, jp, cam, centers, valid, B, J, h, w, r["cube"], (8000.0, 8000.0, 2000.0), img, 28)
        else:
            _lib.unproject_fwd(views, layout, jp, cam, centers, valid, B, J, h, w, r["cube"], (8000.0, 8000.0, 2000.0), img, **kw)
        torch.cuda.synchronize()
    print("issued", len(requests()), "requests")


def parse(trace, out):
    with open(trace, newline="") as fh:
        rows = sorted(csv.DictReader(fh), key=lambda d: int(d["Dispatch_Id"]))
    rq = requests()
    table, cur = {}, -1
    for d in rows:
        name = d["Kernel_Name"]
        if "stamp_kernel" in name:
            cur += 1
            table[rq[cur]["id"]] = []
        elif "unproject_" in name and cur >= 0:
            wg = [int(d["Workgroup_Size_" + a]) for a in "XYZ"]
            grid = [int(d["Grid_Size_" + a]) for a in "XYZ"]
            short = re.sub(r"\(.*$", "", name.replace("sp3d::", "")).replace("void ", "").strip()
            table[rq[cur]["id"]].append(dict(name=short, workgroups=(grid[0] // wg[0]) * (grid[1] // wg[1]) * (grid[2] // wg[2]),
                                             block=wg[0] * wg[1] * wg[2], lds=int(d["LDS_Block_Size"])))
    assert cur + 1 == len(rq), (cur + 1, len(rq))
    with open(out, "w") as fh:
        fh.write("{\n" + ",\n".join(f' "{k}": {json.dumps(v)}' for k, v in table.items()) + "\n}\n")
    print("wrote", out, len(table), "requests,", sum(len(v) for v in table.values()), "dispatches")


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run()
    else:
        parse(sys.argv[2], sys.argv[3])
