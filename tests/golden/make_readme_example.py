"""Writes tests/golden/readme_example.json: SHA-256 digests of the code lines of Klara.jl's README example (the first julia block, sampling
from an unnormalized normal target, and its `reset(job, x)` continuation), one per line after the normalisation
tests/test_host_api.py::test_readme_script_runs_with_two_constructor_swaps applies (comments dropped, whitespace collapsed, empty lines
skipped).  Digests only, no text: the test recovers the README's lines from INTEGRATION.md's snippet by undoing the constructor swaps and
compares digests.  Usage: python tests/golden/make_readme_example.py <Klara.jl checkout>"""
import hashlib
import json
import re
import sys
from pathlib import Path

CLOSURE = "plogtarget(z::Vector{Float64}) ="       # the log-target closure: the one line the snippet states as a device target family instead

readme = (Path(sys.argv[1]) / "README.md").read_text()
blocks = re.findall(r"```julia\n(.*?)```", readme, re.S)
assert "reset(job, [3.2, 9.4])" in blocks[1]
lines = [re.sub(r"\s+", " ", l.split("#")[0]).strip() for l in (blocks[0] + blocks[1]).splitlines() if l.split("#")[0].strip()]
closure = [i for i, l in enumerate(lines) if l.startswith(CLOSURE)]
assert len(closure) == 1 and "using Klara" in lines
out = Path(__file__).resolve().parent / "readme_example.json"
out.write_text(json.dumps({
    "source": "Klara.jl README.md: the first julia block and its reset(job, x) continuation; SHA-256 of each code line (comments dropped, "
              "whitespace collapsed, empty lines skipped), in order",
    "closure_line": closure[0],
    "sha256": [hashlib.sha256(l.encode()).hexdigest() for l in lines],
}, indent=1) + "\n")
print(len(lines), "lines, closure at", closure[0])
