"""Did a change touch any kernel?  python scripts/compare_kernels.py [--bytes] OLD_LIB NEW_LIB
Extracts the gfx950 code object of two builds of libsadvio_ba.so and compares the sorted kernel symbols and, per kernel, the code
size and the register / scratch / LDS figures of its metadata. Prints the differences, or "identical, N kernels".
--bytes also prints which kernels' code bytes differ (a hash of the kernel's slice of .text). For information only: the exit status
does not depend on it. A kernel that calls out-of-line functions (k_solve, k_line_eval) does so through pc-relative offsets, so its
bytes move whenever anything in front of it changes size."""
import hashlib, re, subprocess, sys, tempfile
LLVM = "/opt/rocm/lib/llvm/bin/"
TARGET = "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"
KEYS = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "kernarg_segment_size", "max_flat_workgroup_size"]


def read(tmp, lib):
    co = f"{tmp}/k.co"
    # the fat binary sits in the .hip_fatbin section of the host library
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, f"{tmp}/fat.bin"], check=True)
    subprocess.run([LLVM + "clang-offload-bundler", "--type=o", TARGET, f"--input={tmp}/fat.bin", f"--output={co}", "--unbundle"], check=True)
    symbols = subprocess.run([LLVM + "llvm-readelf", "--symbols", "--wide", co], capture_output=True, text=True, check=True).stdout
    notes = subprocess.run([LLVM + "llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout
    sections = subprocess.run([LLVM + "llvm-readelf", "--sections", "--wide", co], capture_output=True, text=True, check=True).stdout
    # "[ 7] .text PROGBITS <address> <file offset> <size> ..."
    addr, off, size = (int(x, 16) for x in re.search(r"\]\s+\.text\s+PROGBITS\s+(\S+)\s+(\S+)\s+(\S+)", sections).groups())
    with open(co, "rb") as f:
        f.seek(off)
        text = f.read(size)
    return symbols, notes, addr, text


def kernels(lib):
    with tempfile.TemporaryDirectory() as tmp:
        symbols, notes, text_addr, text = read(tmp, lib)
    size, digest = {}, {}
    for ln in symbols.splitlines():
        f = ln.split()
        if len(f) == 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2])
            start = int(f[1], 16) - text_addr
            digest[f[7]] = hashlib.sha256(text[start:start + int(f[2])]).hexdigest()
    out = {}
    # one list entry per kernel under amdhsa.kernels ("  - "), its own keys in any order at that level (the arguments' sit deeper)
    section = re.search(r"(?ms)^amdhsa\.kernels:\n(.*?)^(?=\S)", notes).group(1)   # up to the next top-level key
    for blk in re.split(r"(?m)^  - ", section)[1:]:
        key = lambda k: re.search(rf"(?m)^(?:    )?\.{k}:\s+(\S+)", blk).group(1)
        name = key("name")
        out[name] = {k: int(key(k)) for k in KEYS}
        out[name]["code_bytes"] = size[name]
    return out, {n: digest[n] for n in out}


args = [a for a in sys.argv[1:] if a != "--bytes"]
(old, old_digest), (new, new_digest) = kernels(args[0]), kernels(args[1])
diff = [f"only in {which}: {n}" for which, a, b in (("old", old, new), ("new", new, old)) for n in sorted(a) if n not in b]
for n in sorted(set(old) & set(new)):
    diff += [f"{n}: {k} {old[n][k]} -> {new[n][k]}" for k in old[n] if old[n][k] != new[n][k]]
print("\n".join(diff) if diff else f"identical, {len(new)} kernels")
if "--bytes" in sys.argv[1:]:
    moved = [n for n in sorted(set(old) & set(new)) if old_digest[n] != new_digest[n]]
    print(f"code bytes differ in {len(moved)} of {len(set(old) & set(new))} kernels" + "".join(f"\n  bytes differ: {n}" for n in moved))
sys.exit(1 if diff else 0)
