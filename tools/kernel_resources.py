#!/usr/bin/env python3
"""VGPRs, spilled VGPRs and scratch bytes per lane of every kernel of a built
libpsn_lk.so, from the gfx950 code objects' metadata (no GPU): the .hip_fatbin
section's offload bundles, each code object through llvm-readelf --notes.
Usage: tools/kernel_resources.py [lib] [kernel-regex]
       tools/kernel_resources.py --compare libA libB [kernel-regex]
The second form compares two builds kernel by kernel (resources, code bytes, equality
of the symbols' .text bytes, instruction counts) and prints a JSON table."""
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib):
    with tempfile.TemporaryDirectory() as d:
        fb = os.path.join(d, "fb.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fb}", lib, os.path.join(d, "x.so")],
                       check=True)
        data = open(fb, "rb").read()
    pos = 0
    while True:
        b = data.find(MAGIC, pos)
        if b < 0:
            return
        n = struct.unpack_from("<Q", data, b + 24)[0]
        p = b + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                yield data[b + off:b + off + size]
        pos = b + len(MAGIC)


def kernels(lib):
    out = {}
    for co in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", f.name], capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.agpr_count", txt)[1:]:
            def g(k):
                m = re.search(r"\." + k + r":\s+(\S+)", blk)
                return m.group(1) if m else "?"
            out[g("name")] = {"vgpr": g("vgpr_count"), "vgpr_spill": g("vgpr_spill_count"),
                              "scratch": g("private_segment_fixed_size"), "lds": g("group_segment_fixed_size")}
    return out


def pretty(mangled):
    """The box kernel's builds by the name _lib.kernel_of_tag gives their launches:
    lk_kernel_bx<8, true, 128> for _ZN3psn12lk_kernel_bxILi8ELb1ELi128EEEvNS_12LkLaunchArgsE (the
    builds of 256 threads drop the default size), the forward entry lk_kernel_fw likewise;
    other kernels keep the mangled name."""
    m = re.search(r"lk_kernel_(bx|fw)ILi(\d+)ELb([01])ELi(\d+)E", mangled)
    if not m:
        return mangled
    upt, notail, nt = int(m.group(2)), m.group(3) == "1", int(m.group(4))
    return f"lk_kernel_{m.group(1)}<{upt}, {'true' if notail else 'false'}" + (">" if nt == 256 else f", {nt}>")


def kernel_text(lib, rx):
    """{kernel: (its .text bytes, its instruction count)} of the kernels matching rx: the
    symbol's range by llvm-readelf -S -s, the count from llvm-objdump's disassembly of it."""
    out = {}
    for co in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.run([f"{LLVM}/llvm-readelf", "-S", "-s", "-W", f.name], capture_output=True,
                                 text=True).stdout
            m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", txt)
            if not m:
                continue
            addr, off = int(m.group(1), 16), int(m.group(2), 16)
            for s in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\d+\s+(\S+)$", txt, re.M):
                name, v, size = s.group(3), int(s.group(1), 16), int(s.group(2))
                if name.endswith(".kd") or not (re.search(rx, name) or re.search(rx, pretty(name))):
                    continue
                dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", f"--disassemble-symbols={name}", f.name],
                                     capture_output=True, text=True).stdout
                out[name] = (co[off + v - addr:off + v - addr + size], sum(" // " in ln for ln in dis.splitlines()))
    return out


def compare(lib_a, lib_b, rx):
    """Per kernel of either library matching rx: resources, code bytes and instruction counts of
    both builds (None where a build lacks the kernel), and whether the .text bytes are equal."""
    ra, rb, ta, tb = kernels(lib_a), kernels(lib_b), kernel_text(lib_a, rx), kernel_text(lib_b, rx)
    rows = []
    for n in sorted(set(ta) | set(tb)):
        a, b = ta.get(n), tb.get(n)
        rows.append({"kernel": pretty(n), "mangled": n, "resources_a": ra.get(n), "resources_b": rb.get(n),
                     "resources_equal": ra.get(n) == rb.get(n), "code_bytes_a": a and len(a[0]),
                     "code_bytes_b": b and len(b[0]), "text_equal": bool(a and b and a[0] == b[0]),
                     "instructions_a": a and a[1], "instructions_b": b and b[1]})
    return rows


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--compare":  # --compare libA libB [kernel-regex]: a JSON table
        import json
        print(json.dumps(compare(sys.argv[2], sys.argv[3], sys.argv[4] if len(sys.argv) > 4 else "lk_kernel"), indent=1))
        sys.exit(0)
    lib = sys.argv[1] if len(sys.argv) > 1 else "mcmtt_opticalflow_amd/lib/libpsn_lk.so"
    rx = sys.argv[2] if len(sys.argv) > 2 else "lk_kernel"
    for n, r in sorted(kernels(lib).items()):
        if re.search(rx, n) or re.search(rx, pretty(n)):
            print(f"{pretty(n):56s} vgpr {r['vgpr']:>4s} spill {r['vgpr_spill']:>3s} scratch {r['scratch']:>4s}")
