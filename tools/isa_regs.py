#!/usr/bin/env python3
"""Register counts of every kernel of libtrh as the ISA declares them (.vgpr_count / .sgpr_count / scratch / LDS of the code objects'
metadata notes), for the profile summaries: rocprofv3's `vgpr_count` column is an allocation-granule count on gfx950 (80 for a kernel
whose ISA says 160), which VERDICT r03 asked to print beside the real figure.
    tools/isa_regs.py            -> profiles/isa_registers.json  {kernel<Field>: {"vgpr": .., "sgpr": .., "scratch": .., "lds": ..}}
Runs in the build container (llvm tools of /opt/rocm); the extracted bundles go to a temporary directory."""
import glob, json, os, re, shutil, subprocess, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def short(name):
    m = re.search(r"(\w+_kernel)\b", name)
    if m:
        t = re.search(r"<trh::(\w+)Params", name)
        return m.group(1) + (f"<{t.group(1)}>" if t else "")
    return name.split("(")[0][-60:]


def collect(count_instructions=True):
    """{kernel<Field>: {"vgpr", "sgpr", "scratch", "lds", "isa_instructions"}} of the objects `make` left in csrc/ (read only); without
    count_instructions the code objects are not disassembled and isa_instructions is 0"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sorted(glob.glob(os.path.join(ROOT, "tiny-ram-halo2_amd", "csrc", "*.o"))):
            local = os.path.join(tmp, os.path.basename(obj))
            shutil.copy(obj, local)
            subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", local], capture_output=True)
            for co in glob.glob(local + ".*amdgcn*"):
                notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
                # static instruction count per kernel: lines of the disassembly between the kernel's label and the next one
                counts, cur_fn = {}, None
                for line in subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True).stdout.splitlines() if count_instructions else []:
                    m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
                    if m:
                        cur_fn = m.group(1)
                        counts[cur_fn] = 0
                    elif cur_fn and re.match(r"^\s+[a-z_0-9]+(\s|$)", line) and not line.strip().startswith("s_code_end"):
                        counts[cur_fn] += 1
                # one block of the notes per kernel; the order of its keys is the YAML emitter's (alphabetical: .group_segment_fixed_size comes
                # before .name), so a block ends where a key repeats or the notes end -- not at .name
                def emit(cur):
                    if not all(k in cur for k in ("short", "vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")):
                        return
                    prev = out.get(cur["short"])
                    ent = {"vgpr": cur["vgpr_count"], "sgpr": cur["sgpr_count"], "scratch": cur["private_segment_fixed_size"], "lds": cur["group_segment_fixed_size"],
                           "isa_instructions": counts.get(cur["mangled"].replace(".kd", ""), 0)}
                    if prev is None or ent["vgpr"] > prev["vgpr"]:
                        out[cur["short"]] = ent  # template instances that share a short name: the largest
                cur = {}
                for line in notes.splitlines():
                    m = re.match(r"    \.(name|vgpr_count|sgpr_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)", line)
                    if not m:
                        continue
                    key, val = m.group(1), m.group(2)
                    if key in cur:
                        emit(cur)
                        cur = {}
                    if key == "name":
                        cur["name"] = cur["mangled"] = val
                        cur["short"] = short(subprocess.run(["c++filt", val], capture_output=True, text=True).stdout.strip())
                    else:
                        cur[key] = int(val)
                emit(cur)
    return out


def main():
    out = collect()
    path = os.path.join(ROOT, "profiles", "isa_registers.json")
    json.dump(dict(sorted(out.items())), open(path, "w"), indent=1)
    print(f"{len(out)} kernels -> {path}")
    for k in ("msm_accumulate_seg_kernel<Fp>", "msm_combine_kernel<Fp>", "msm_reduce_kernel<Fp>", "ntt_passy_kernel<Fp>"):
        print(k, out.get(k))


if __name__ == "__main__":
    main()
