#!/usr/bin/env python3
"""Resource usage of the gm_step_kernel instantiations in a compiled gm_capi object, read from
the gfx950 code object's metadata (no GPU needed): VGPRs, SGPRs, LDS bytes, scratch bytes per
lane and code size of each kernel, plus the code size of named device functions.

Compare two trees ("PPO actor-critic rollout"):
  python -c "import __graft_entry__ as g; g.build()"        # in each tree
  python tools/step_kernel_resources.py --label parent --label this --out profiles/ac_rollout_step_kernel_resources.json \\
         <parent tree>/gripper-mujoco_amd/lib/obj/gm_capi.hip.o gripper-mujoco_amd/lib/obj/gm_capi.hip.o
The script exits 1 when the last object's LDS or scratch exceeds the first's for any kernel.

Prove that a change which only moves source text left the device code alone:
  python tools/step_kernel_resources.py --same-code <parent>/.../obj/gm_capi.hip.o gripper-mujoco_amd/lib/obj/gm_capi.hip.o
compares the .text, .rodata and .note sections of the two gfx950 code objects byte for byte
(the symbol tables may be ordered differently; nothing else may) and exits 1 on a difference."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
SECTIONS = (".text", ".rodata", ".note")
FUNCS = ("ac_rollout_driver", "replay_record", "ga_sample", "gm_ac_kernel", "gm_ac_gae_kernel", "gm_policy_kernel",
         "gm_td_target_kernel", "gm_replay_sample_kernel", "gm_learn_grad_kernel", "gm_learn_step_kernel",
         "substep_loop", "reset_env", "driver_actions", "sac_rollout_driver", "gs_sample", "gm_sac_actor_kernel",
         "gm_sac_q_kernel", "gm_sac_push_begin_kernel", "gm_sac_replay_sample_kernel")


def tool(name, *args):
    return subprocess.run([os.path.join(LLVM, name), *args], check=True, capture_output=True, text=True).stdout


def usage(obj):
    with tempfile.TemporaryDirectory() as d:
        co = code_object(obj, d)
        notes = tool("llvm-readelf", "--notes", co)
        syms = tool("llvm-readelf", "-sW", co)
    size = {}
    for line in syms.splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2])
    kernels = {}
    for blk in notes.split("- .agpr_count")[1:]:
        def g(key):
            return re.search(r"\." + key + r":\s+(\S+)", blk).group(1)
        name = g("name")
        if "gm_step_kernel" not in name:
            continue
        m = re.search(r"gm_step_kernelILi(\d+)ELb(\d)ELb(\d)E", name)
        short = f"CL={m.group(1)} CAL={m.group(2)} DUO={m.group(3)}" if m else name
        kernels[short] = dict(vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")),
                              lds_bytes=int(g("group_segment_fixed_size")),
                              scratch_bytes_per_lane=int(g("private_segment_fixed_size")), code_bytes=size.get(name))
    funcs = {}
    for f in FUNCS:   # a template's instantiations go by their symbols
        hits = {s: n for s, n in size.items() if re.search(r"(?<![A-Za-z_])" + re.escape(f), s)}   # (not a longer name's tail)
        funcs.update({f: n for n in hits.values()} if len(hits) == 1 else hits)
    return dict(kernels=kernels, functions=funcs)


def code_object(obj, d):
    fat, co = os.path.join(d, "fat"), os.path.join(d, "co")
    tool("llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj)
    tool("clang-offload-bundler", "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}")
    return co


def same_code(a, b):
    """Byte comparison of the code-bearing sections of two objects' gfx950 code objects; a report
    line per section, the first differing section with the function its first differing byte is in."""
    lines, first = [], None
    with tempfile.TemporaryDirectory() as d:
        cos = []
        for i, obj in enumerate((a, b)):
            os.mkdir(os.path.join(d, str(i)))
            cos.append(code_object(obj, os.path.join(d, str(i))))
        for sec in SECTIONS:
            data = []
            for i, co in enumerate(cos):
                out = os.path.join(d, str(i), "sec")
                tool("llvm-objcopy", "--dump-section", f"{sec}={out}", co)
                with open(out, "rb") as f:
                    data.append(f.read())
            same = data[0] == data[1]
            lines.append(f"{sec:8s} {len(data[0]):9d} B  {len(data[1]):9d} B  {'identical' if same else 'DIFFERENT'}")
            if same or first is not None:
                continue
            off = next((k for k, (x, y) in enumerate(zip(*data)) if x != y), min(map(len, data)))
            first = f"first difference: {sec} + {off:#x}"
            if sec == ".text":   # the function of the first object that holds that byte
                base = int(re.search(r"\] \.text\s+\S+\s+([0-9a-f]+)", tool("llvm-readelf", "-SW", cos[0])).group(1), 16)
                for f in (ln.split() for ln in tool("llvm-readelf", "-sW", cos[0]).splitlines()):
                    if len(f) >= 8 and f[3] == "FUNC" and int(f[1], 16) <= base + off < int(f[1], 16) + int(f[2]):
                        first += f" in {f[7]}"
                        break
    return lines, first


def main():
    if "--same-code" in sys.argv[1:]:
        ap = argparse.ArgumentParser()
        ap.add_argument("--same-code", nargs=2, metavar=("PARENT_OBJ", "OBJ"), required=True)
        ap.add_argument("--out", help="append the report to this file")
        a = ap.parse_args()
        lines, first = same_code(*a.same_code)
        text = "\n".join([f"{a.same_code[0]} vs {a.same_code[1]}", *lines, first or "same code"]) + "\n"
        if a.out:
            with open(a.out, "a") as f:
                f.write(text)
        print(text, end="")
        return 1 if first else 0
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", action="append", default=[])
    ap.add_argument("--out")
    ap.add_argument("objects", nargs="+")
    a = ap.parse_intermixed_args()
    labels = a.label + [os.path.basename(o) for o in a.objects[len(a.label):]]
    res = {lab: usage(obj) for lab, obj in zip(labels, a.objects)}
    grew = []
    if len(labels) > 1:
        first, last = res[labels[0]]["kernels"], res[labels[-1]]["kernels"]
        for k in sorted(first):
            for field in ("lds_bytes", "scratch_bytes_per_lane"):
                if k in last and last[k][field] > first[k][field]:
                    grew.append(f"{k} {field} {first[k][field]} -> {last[k][field]}")
        res["lds_or_scratch_grew"] = grew
    text = json.dumps(res, indent=1, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    return 1 if grew else 0


if __name__ == "__main__":
    sys.exit(main())
