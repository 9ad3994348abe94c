#!/usr/bin/env python3
"""Is the gfx950 machine code of two builds the same, function by function?  (CPU only.)

    python scripts/isa_diff.py old/vit.o new/vit.o        # host objects with a .hip_fatbin section, or bare code objects
    python scripts/isa_diff.py old/vit.o new/vit.o --rename REGEX REPLACEMENT   # re.sub on the OLD symbols first (a template that
                                                                                # gained a defaulted argument changes its mangled names)

Unbundles the gfx950 code object (the objcopy + clang-offload-bundler recipe of tests/test_abi.py::test_m0_users and
scripts/kernel_resources.sh), disassembles it and compares, per function symbol, the instruction list -- addresses and
encodings dropped; s_call targets and the pc-relative literal behind an s_getpc_b64 (s_add_u32 / s_addc_u32 sN, sN, 0x...)
replaced by a placeholder, and the s_nop 0 padding behind a function's last instruction dropped, because they move when ANOTHER
function changes size; branches inside a function are pc-relative and stay as they are -- and, per kernel, the register, spill, LDS and scratch figures of the metadata notes.  Prints the
functions that differ; exit status 1 if any do."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
NOTES = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
         ".private_segment_fixed_size")


def code_object(path, tmp):
    with open(path, "rb") as fh:
        if fh.read(20)[18:20] == b"\xe0\x00":   # e_machine = EM_AMDGPU: already a code object
            return path
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, os.path.basename(path) + ".co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, fat], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--targets={TARGET}", f"--input={fat}", f"--output={co}",
                    "--unbundle"], check=True)
    return co


def functions(co):
    """{symbol: [normalised instruction, ...]}"""
    asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    out, cur, pc_regs = {}, None, set()
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
        if m:
            cur, pc_regs = out.setdefault(m.group(1), []), set()
            continue
        ins = " ".join(line.split("//")[0].split())
        if cur is None or not ins:
            continue
        m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", ins)
        if m:
            pc_regs = {f"s{m.group(1)}", f"s{m.group(2)}"}
        m = re.match(r"(s_addc?_u32) (s\d+), (s\d+), (0x[0-9a-f]+|-?\d+)$", ins)
        if m and m.group(2) == m.group(3) and m.group(2) in pc_regs:
            pc_regs.discard(m.group(2))
            ins = f"{m.group(1)} {m.group(2)}, {m.group(3)}, <pcrel>"
        ins = re.sub(r"^(s_call_b64 s\[\d+:\d+\]), .*", r"\1, <target>", ins)
        cur.append(ins)
    for body in out.values():   # alignment padding in front of the next symbol: it moves with the function's address
        while body and body[-1] in ("s_nop 0", "...", "s_code_end"):
            body.pop()
    return out


def resources(co):
    """{kernel symbol: {note: value}}; the notes of a kernel are sorted by key: .wavefront_size closes it"""
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    out, cur, symbol = {}, {}, None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*(\.\w+):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) in NOTES:
            cur[m.group(1)] = m.group(2)
        elif m.group(1) == ".symbol":
            symbol = re.sub(r"\.kd$", "", m.group(2).strip("'\""))
        elif m.group(1) == ".wavefront_size":
            out[symbol], cur = cur, {}
    return out


def main(old, new, rename=None):
    with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1:
        co0, co1 = code_object(old, t0), code_object(new, t1)
        f0, f1, r0, r1 = functions(co0), functions(co1), resources(co0), resources(co1)
    if rename:   # a template that gained a defaulted argument: the old symbols under their new names
        f0 = {re.sub(rename[0], rename[1], k): v for k, v in f0.items()}
        r0 = {re.sub(rename[0], rename[1], k): v for k, v in r0.items()}
    bad = 0
    for name in sorted(set(f0) | set(f1)):
        if name not in f0 or name not in f1:
            why = "only in " + (old if name in f0 else new)
        elif f0[name] != f1[name]:
            first = next((i for i, (a, b) in enumerate(zip(f0[name], f1[name])) if a != b), min(len(f0[name]), len(f1[name])))
            why = f"instructions differ: {len(f0[name])} -> {len(f1[name])}, first at #{first}"
        elif r0.get(name) != r1.get(name):
            why = f"resources differ: {r0.get(name)} -> {r1.get(name)}"
        else:
            continue
        bad += 1
        print(f"DIFF {name}: {why}")
    print(f"{len(set(f0) | set(f1))} functions ({len(r1)} kernels with resource notes) compared, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[3] == "--rename":
        sys.exit(main(sys.argv[1], sys.argv[2], (sys.argv[4], sys.argv[5])))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
