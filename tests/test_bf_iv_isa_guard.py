"""Build-time guard for the interval probe sweep (csrc/nts_bf_iv.inc k_bf_count_intervals): it is in the gfx950 code object of both
built libraries exactly once, keeps nothing in scratch memory, spills no register, stages what the sketch's sweep stages (at most
10 KB of LDS) and stays within 64 vector registers -- eight waves per SIMD, the occupancy docs/design/04_9_gap_content.md counts on
for its probes in flight."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBS = [os.path.join(ROOT, "ntsynt_amd", n) for n in ("libntsynt_hip.so", "libntsynt_hip_exp.so")]
LLVM = "/opt/rocm/lib/llvm/bin"
VGPR_CEILING = 64


def _notes(lib, d):
    assert os.path.exists(lib), f"{os.path.basename(lib)} is not built (__graft_entry__.build())"
    for tool in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf"):
        assert os.path.exists(os.path.join(LLVM, tool)), f"{tool} not in {LLVM}"
    fat, co = str(d / "fat.bin"), str(d / "dev.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib, str(d / "unused.so")], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                    "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], check=True)
    return subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout


def _kernel_meta(notes, symbol):
    at = notes.index(f".name:           {symbol}\n")
    start = notes.rfind("  - .agpr_count", 0, at)
    if start < 0:
        start = notes.rfind("  - .args", 0, at)
    end = notes.find("\n  - ", at)
    block = notes[start:end if end > 0 else None]
    return {m.group(1): m.group(2) for m in re.finditer(r"\.(\w+):\s+(\S+)", block)}


@pytest.mark.parametrize("lib", LIBS, ids=["product", "experiments"])
def test_interval_probe_sweep_is_in_the_code_object_without_scratch_or_spills(lib, tmp_path):
    notes = _notes(lib, tmp_path)
    found = re.findall(r"\.name:\s+(\S*k_bf_count_intervals\S*)\n", notes)
    assert len(found) == 1, found
    m = _kernel_meta(notes, found[0])
    print(os.path.basename(lib), {key: m.get(key) for key in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size")})
    assert m["private_segment_fixed_size"] == "0", m
    assert m.get("vgpr_spill_count", "0") == "0" and m.get("sgpr_spill_count", "0") == "0", m
    assert int(m["group_segment_fixed_size"]) <= 10 * 1024, m
    assert int(m["vgpr_count"]) + int(m.get("agpr_count", "0")) <= VGPR_CEILING, m
