"""Kernel resource table of the built library: every gfx950 code object inside libphysics_hip.so's .hip_fatbin,
its kernels and their scratch (private segment), LDS, VGPR and SGPR use.

    python tools/code_objects.py [path/to/libphysics_hip.so]
    python tools/code_objects.py --diff OTHER.so [path/to/libphysics_hip.so]

--diff: per kernel, whether the disassembly (instruction text without addresses and comments) equals OTHER.so's; where it
does not, the instruction counts and VGPR, SGPR, LDS and scratch of both, OTHER's first.

Used by tests/test_build_rules.py for the "no kernel uses scratch memory" rule."""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _fatbin(lib):
    # a library of host code alone (tests/cpp/libcolor_probe.so) has no fat binary: no code objects, nothing to hold to a rule
    sections = subprocess.run([f"{LLVM}/llvm-readelf", "--sections", lib], check=True, capture_output=True, text=True).stdout
    if ".hip_fatbin" not in sections:
        return b""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={out}", lib, os.path.join(d, "copy.so")], check=True)
        return open(out, "rb").read()


def code_objects(lib):
    """Yield the device ELF images (bytes) of every bundle in the library's fat binary."""
    blob = _fatbin(lib)
    at = blob.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "amdgcn" in triple and size:
                yield blob[at + off:at + off + size]
        at = blob.find(MAGIC, at + len(MAGIC))


def kernels(lib):
    """[{name, scratch, lds, vgprs, sgprs, spills}] for every kernel in the library."""
    out = []
    for image in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(image)
            f.flush()
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", f.name], check=True, capture_output=True, text=True).stdout
        for block in notes.split("  - .agpr_count:")[1:]:
            def field(key, block=block):
                m = re.search(rf"\.{key}:\s+(\S+)", block)
                return m.group(1) if m else None
            out.append({"name": field("name"), "scratch": int(field("private_segment_fixed_size")),
                        "lds": int(field("group_segment_fixed_size")), "vgprs": int(field("vgpr_count")),
                        "sgprs": int(field("sgpr_count")), "spills": int(field("vgpr_spill_count"))})
    return out


def count_instructions(lib, mnemonics):
    """Occurrences of the given mnemonics in the disassembly of every code object of the library."""
    total = 0
    for image in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(image)
            f.flush()
            text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", f.name], check=True, capture_output=True, text=True).stdout
        total += sum(text.count(m) for m in mnemonics)
    return total


def disassembly(lib):
    """{kernel name: [instruction text without addresses and comments]} of every kernel in the library."""
    names = {k["name"] for k in kernels(lib)}
    out, cur = {}, None
    for image in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".elf") as f:
            f.write(image)
            f.flush()
            text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", f.name], check=True,
                                  capture_output=True, text=True).stdout
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]* ?<(.+)>:$", line)
            if m:
                cur = out.setdefault(m.group(1), []) if m.group(1) in names else None
            elif cur is not None and line.startswith(("\t", " ")) and line.strip():
                cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def diff(lib, other):
    """Print the --diff table; returns the number of kernels whose disassembly differs or that only one side has."""
    mine, theirs = disassembly(lib), disassembly(other)
    res = {side: {k["name"]: k for k in kernels(path)} for side, path in (("mine", lib), ("theirs", other))}
    differ = 0
    for name in sorted(set(mine) | set(theirs)):
        short = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.split("(")[0].strip()[:70]
        if name not in mine or name not in theirs:
            differ += 1
            print(f"{short:70s} only in {'this library' if name in mine else 'OTHER'}")
        elif mine[name] == theirs[name]:
            print(f"{short:70s} identical ({len(mine[name])} instructions)")
        else:
            differ += 1
            a, b = res["theirs"][name], res["mine"][name]
            print(f"{short:70s} DIFFERS: instructions {len(theirs[name])} -> {len(mine[name])}, vgprs {a['vgprs']} -> {b['vgprs']}, "
                  f"sgprs {a['sgprs']} -> {b['sgprs']}, lds {a['lds']} -> {b['lds']}, scratch {a['scratch']} -> {b['scratch']}")
    print(f"{len(set(mine) | set(theirs))} kernels, {differ} differ")
    return differ


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    args = [a for a in sys.argv[1:] if a != "--check"]
    other = None
    if "--diff" in args:
        at = args.index("--diff")
        other = args[at + 1]
        del args[at:at + 2]
    lib = args[0] if args else os.path.join(here, "..", "physics_amd", "csrc", "libphysics_hip.so")
    if "--check" in sys.argv:
        # the build's own gate (csrc/Makefile): the two rules of DESIGN.md section 8 hold on the code objects just linked,
        # or the build FAILS - a compiler update that drops the -packed-fp32-ops feature must not pass as a warning
        packed = count_instructions(lib, ("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32"))
        bad = [(k["name"], k["scratch"], k["spills"]) for k in kernels(lib) if k["scratch"] or k["spills"]]
        if packed or bad:
            print(f"code object rules violated: {packed} packed fp32 arithmetic instructions; scratch / spills: {bad}", file=sys.stderr)
            sys.exit(1)
        sys.exit(0)
    if other:
        diff(lib, other)
        sys.exit(0)
    ks = kernels(lib)
    for k in sorted(ks, key=lambda k: k["name"]):
        short = subprocess.run(["c++filt", k["name"]], capture_output=True, text=True).stdout.split("(")[0].strip()
        print(f"{short[:60]:60s} scratch {k['scratch']:4d}  lds {k['lds']:7d}  vgprs {k['vgprs']:4d}  sgprs {k['sgprs']:4d}  spills {k['spills']}")
    print(f"{len(ks)} kernels; packed fp32 arithmetic instructions:", count_instructions(lib, ("v_pk_mul_f32", "v_pk_add_f32", "v_pk_fma_f32")))
