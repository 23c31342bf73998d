"""The gfx950 code objects of a built library: what the metadata notes say about
each kernel.  Reads the notes only (llvm-objcopy, clang-offload-bundler,
llvm-readelf of the ROCm LLVM tools); never looks at instructions."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gqmap-opticalflow_amd", "libgqmap.so")
LLVM = "/opt/rocm/lib/llvm/bin"
KEYS = ("vgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count")


def available(lib=LIB):
    return os.path.exists(lib) and bool(shutil.which(f"{LLVM}/llvm-readelf"))


@functools.lru_cache(maxsize=None)
def kernels(lib=LIB):
    """{mangled kernel name: {key of KEYS: int}} over every translation unit of lib; agpr_count reads 0 where the
    notes do not carry it, any other key must be there."""
    seen = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", lib, os.path.join(tmp, "x.so")],
                       check=True, capture_output=True)
        # one bundle per translation unit, each behind the bundler's magic string
        with open(fat, "rb") as fh:
            blob = fh.read()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", blob)]
        for i, (a, b) in enumerate(zip(starts, starts[1:] + [len(blob)])):
            part, co = os.path.join(tmp, f"part{i}.bin"), os.path.join(tmp, f"co{i}.elf")
            with open(part, "wb") as fh:
                fh.write(blob[a:b])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={part}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True,
                           capture_output=True)
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                                   text=True).stdout
            for block in re.split(r"\n  - ", notes):
                name = re.search(r"\n\s*\.name:\s+(\S+)", "\n" + block)
                if not name or not re.search(r"\.vgpr_count:\s+\d+", block):
                    continue
                found = {key: re.search(rf"\.{key}:\s+(\d+)", block) for key in KEYS}
                missing = [key for key, m in found.items() if not m and key != "agpr_count"]
                assert not missing, (name.group(1), missing)
                seen[name.group(1)] = {key: int(m.group(1)) if m else 0 for key, m in found.items()}
    return seen
