"""Compile-time gate of the zero-variance kernels (csrc/klara_zv.hip), no GPU needed: every k_zv_* kernel of the gfx950 code object uses
0 bytes of scratch and spills no vector register, and the instantiations that hold 13 accumulator tiles per wavefront stay within the 256
registers a workgroup of 8 wavefronts leaves each of them (2 wavefronts per SIMD).  Compiled with the Makefile's own flags."""
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "klara.jl_amd" / "csrc"


def _makefile_flags():
    mk = (CSRC / "Makefile").read_text()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, re.M).group(1).split()
    arch = re.search(r"^ARCH \?= (\S+)$", mk, re.M).group(1)
    assert arch == "gfx950" and "-O3" in flags and "-ffp-contract=off" in flags
    assert "klara_zv.hip" in mk[mk.index("SRCS ="):mk.index("DIAGT_SRCS =")]
    return arch, flags


def test_zv_kernels_use_no_scratch_and_fit_their_wavefronts(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert Path(hipcc).exists(), "hipcc is what builds the library: it must be there"
    arch, flags = _makefile_flags()
    out = tmp_path / "klara_zv.s"
    r = subprocess.run([hipcc, f"--offload-arch={arch}", *flags, "-S", "--cuda-device-only", "-o", str(out), str(CSRC / "klara_zv.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = {}
    for blk in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", out.read_text(), re.S):
        t = blk.group(0)
        name = re.search(r"\.name:\s+(\S+)", t).group(1)
        meta[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", t).group(1))
                      for k in ("vgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count")}
    zv = {k: v for k, v in meta.items() if "k_zv_" in k}
    gram = [k for k in zv if "k_zv_gram" in k]
    apply_ = [k for k in zv if "k_zv_apply" in k]
    # 2 orders x 5 tile counts, 2 orders x 4 k-step counts, the solve and the merge
    assert len(gram) == 10 and len(apply_) == 8 and len(zv) == 20, sorted(zv)
    for name, m in sorted(zv.items()):
        print(name, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        if "k_zv_gram" in name or "k_zv_apply" in name:          # launched as 8 wavefronts: two per SIMD share 512 registers
            assert m["vgpr_count"] <= 256 and m["agpr_count"] <= 256, (name, m)
    wide = [k for k in gram if re.search(r"k_zv_gramILi[12]ELi13EE", k)]
    assert len(wide) == 2, gram
