"""Instruction census of the (j,k) step loop of wino_fused16_kernel from the compiler's assembly: the innermost loop that
holds the 36 matrix instructions, counted by class.  No GPU needed.

    hipcc --offload-arch=gfx950 <the flags of selfpose3d_amd/build.py> --cuda-device-only -S csrc/sp3d_wino_fused.hip -o wf.s
    python tools/count_step_isa.py wf.s [substring of the mangled kernel name ...]
"""
import collections
import json
import re
import sys


def functions(text):
    """{mangled name: [instruction lines and labels]} of every kernel of an AMDGPU assembly file"""
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name and re.match(r"^\s*\.end_amdhsa_kernel|^\.Lfunc_end", line):
            name = None
        if name is not None:
            s = line.split(";")[0].strip()
            if s and not s.startswith("."):
                out[name].append(s)
            elif re.match(r"^\.LBB\d+_\d+:", line):
                out[name].append(line.split(":")[0] + ":")
    return out


def step_loop(body):
    """the shortest label..backward-branch span that contains at least 36 matrix instructions"""
    labels = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
    best = None
    for i, l in enumerate(body):
        m = re.match(r"s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), i) < i:
            span = body[labels[m.group(1)]:i + 1]
            if sum("v_mfma" in s for s in span) >= 36 and (best is None or len(span) < len(best)):
                best = span
    return best


def census(span):
    c = collections.Counter()
    for s in span:
        if s.endswith(":"):
            continue
        op = s.split()[0]
        if "mfma" in op:
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            c["valu:" + re.sub(r"_e(32|64)$", "", op)] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_")):
            c["vmem"] += 1
        elif op.startswith("s_waitcnt") or op.startswith("s_nop"):
            c["wait_nop"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        else:
            c["other"] += 1
    return c


if __name__ == "__main__":
    fns = functions(open(sys.argv[1]).read())
    want = sys.argv[2:] or ["wino_fused16_kernel"]
    for name, body in fns.items():
        if not all(w in name for w in want):
            continue
        span = step_loop(body)
        if span is None:
            continue
        c = census(span)
        top = {k: v for k, v in sorted(c.items()) if not k.startswith("valu:")}
        detail = {k[5:]: v for k, v in sorted(c.items(), key=lambda kv: -kv[1]) if k.startswith("valu:")}
        print(json.dumps({"kernel": name, "step_loop": top, "valu_by_opcode": detail}))
