"""CPU tests of the host-side mirror of the reference API and of the C-ABI library surface."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import klara_jl_amd as K
from klara_jl_amd import _lib as L

ROOT = Path(__file__).resolve().parent.parent
JL = ROOT / "julia" / "KlaraHIP" / "src" / "KlaraHIP.jl"


def test_library_exports_every_declared_symbol(klib):
    header = (ROOT / "include" / "klara_hip.h").read_text()
    # (klara_user_*: the two functions a user-defined target's source defines, named in a comment — not library symbols)
    declared = {n for n in re.findall(r"\b(klara_[a-z0-9_]+)\s*\(", header) if not n.startswith("klara_user_")} - {"klara_status"}
    assert declared == set(L.EXPORTS), declared ^ set(L.EXPORTS)
    for name in declared:
        assert hasattr(klib, name), name
    assert klib.klara_abi_version() == L.KLARA_ABI_VERSION == 6
    # the binding's copies of the header's launch lengths (bench.py and the tests read them from the binding, never a literal)
    defs = dict(re.findall(r"#define (KLARA_DEFAULT_STEPS_PER_LAUNCH(?:_SLICE)?) (\d+)", header))
    assert int(defs["KLARA_DEFAULT_STEPS_PER_LAUNCH"]) == L.DEFAULT_STEPS_PER_LAUNCH and int(defs["KLARA_DEFAULT_STEPS_PER_LAUNCH_SLICE"]) == L.DEFAULT_STEPS_PER_LAUNCH_SLICE


def test_desc_struct_matches_header_layout():
    # 8-byte aligned, no surprises: the struct is what INTEGRATION.md's ccall stub mirrors field by field
    assert C.sizeof(L.KlaraDesc) % 8 == 0
    assert L.KlaraDesc.nchains.offset == 24 and L.KlaraDesc.mh_sigma.offset == 48
    assert L.KlaraDesc.stream.offset == C.sizeof(L.KlaraDesc) - 8


def test_desc_fields_agree_across_header_ctypes_and_julia_stub():
    """struct klara_desc: the C header, the ctypes mirror (klara.jl_amd/_lib.py) and the Julia ccall stub
    (julia/KlaraHIP/src/KlaraHIP.jl) list the same fields in the same order with matching widths."""
    import re
    hdr = (ROOT / "include" / "klara_hip.h").read_text()
    body = hdr[hdr.index("typedef struct klara_desc"):]
    body = body[body.index("{") + 1:body.index("} klara_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    cfields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.match(r"(const )?([A-Za-z_0-9]+)( ?\*)? ?([A-Za-z_0-9]+)$", decl)
        assert m, decl
        ctype = "ptr" if m.group(3) else m.group(2)
        cfields.append((m.group(4), ctype))
    width = {"uint32_t": 4, "int32_t": 4, "int64_t": 8, "uint64_t": 8, "double": 8, "ptr": 8, "void": 8, "char": 8}
    py = [(n, C.sizeof(t)) for n, t in L.KlaraDesc._fields_]
    assert [n for n, _ in cfields] == [n for n, _ in py]
    assert [width[t] for _, t in cfields] == [w for _, w in py]
    jl = JL.read_text()
    jbody = jl[jl.index("struct KlaraDesc") + len("struct KlaraDesc"):]
    jbody = jbody[:jbody.index("\nend")]
    jfields = re.findall(r"([A-Za-z_0-9]+)::([A-Za-z0-9{}]+)", jbody)
    jwidth = {"UInt32": 4, "Int32": 4, "Int64": 8, "UInt64": 8, "Float64": 8, "Ptr{Float64}": 8, "Ptr{Cvoid}": 8, "Cstring": 8}
    assert [n for n, _ in jfields] == [n for n, _ in py]
    assert [jwidth[t] for _, t in jfields] == [w for _, w in py]


def test_julia_job_constructor_maps_klara_structs_to_the_descriptor():
    """julia/KlaraHIP/src/KlaraHIP.jl cannot run here (no Julia), so what can drift is checked mechanically:
    (1) klara_desc(; ...) takes every field of the struct by keyword and passes them positionally in struct order;
    (2) the HIPMCJob constructor reads Klara's own field names — the ones the reference's structs declare (citations in the
        stub) — and sets only descriptor fields that exist;
    (3) every ccall passes as many arguments as its signature tuple names, with the argument count of the C prototype;
    (4) the constants mirror the header."""
    import re
    jl = JL.read_text()
    fields = [n for n, _ in L.KlaraDesc._fields_]
    # (1)
    sig = jl[jl.index("function klara_desc(;") + len("function klara_desc(;"):]
    body = sig[sig.index("KlaraDesc(UInt32(sizeof(KlaraDesc)), KLARA_ABI_VERSION,"):]
    sig = sig[:sig.index(")\n    KlaraDesc(")]
    kws = re.findall(r"([A-Za-z_0-9]+)=", re.sub(r"\([^()]*\)", "", sig))
    assert kws == fields[2:], (kws, fields[2:])
    pos = body[len("KlaraDesc(UInt32(sizeof(KlaraDesc)), KLARA_ABI_VERSION,"):body.index(")\nend")]
    assert [a.strip() for a in pos.replace("\n", " ").split(",")] == fields[2:]
    # (2) Klara field names (reference file:line as cited in the stub) and descriptor keys
    ctor = jl[jl.index("function HIPMCJob(parameter::HIPParameter"):jl.index("# raw form for callers")]
    for klara_field in ("sampler.driftstep", "sampler.leapstep", "sampler.nleaps", "sampler.widths", "sampler.stepout", "sampler.setproposal",
                        "sampler.symmetric", "sampler.normalised", "tn.period", "tn.verbose", "tn.targetrate", "tn.score", "tn.nadapt",
                        "tn.ε0bar", "tn.h0bar", "tn.γ", "tn.t0", "tn.κ", "mcrange.nsteps", "mcrange.burnin", "mcrange.thinning"):
        assert klara_field in ctor, klara_field
    assert "job.range.npoststeps" in jl and "job.range.postrange" in jl and "job.range.nsteps" in jl
    keys = set(re.findall(r"kw\[:([A-Za-z_0-9]+)\]", ctor)) | set(re.findall(r":([A-Za-z_0-9]+) =>", ctor[:ctor.index("# --- sampler")]))
    assert keys <= set(fields), keys - set(fields)
    assert {"sampler", "target", "tuner", "nchains", "ndims", "nsteps", "burnin", "thinning", "monitor", "seed", "driftstep", "leapstep",
            "nleaps", "mh_sigma", "slice_widths", "slice_stepout", "targetrate", "period", "verbose", "da_nadapt", "gauss_prec", "logit_X",
            "hier_Y", "custom_src"} <= keys
    # NState fields the output() fills (nstates/ParameterNStates/BasicContMuvParameterNState.jl:1-21)
    for f in ("ns.value", "ns.logtarget", "ns.gradlogtarget", "ns.loglikelihood", "ns.logprior", "ns.diagnosticvalues"):
        assert f in jl, f
    # (3) ccall arity against the header's prototypes
    hdr = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "klara_hip.h").read_text(), flags=re.S)
    proto = {m.group(1): len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
             for m in re.finditer(r"\b(klara_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr)}
    for m in re.finditer(r"ccall\(\(:(klara_[a-z_0-9]+), lib\), (\w+), \(([^()]*(?:\{[^()]*\}[^()]*)*)\),", jl):
        name, argt = m.group(1), m.group(3)
        n = len([a for a in re.split(r",\s*(?![^{}]*\})", argt) if a.strip()])
        assert proto[name] == n, (name, proto[name], n)
    # (4)
    for name, val in (("SAMPLER_MH", L.SAMPLER_MH), ("SAMPLER_SLICE", L.SAMPLER_SLICE), ("TARGET_CUSTOM", L.TARGET_CUSTOM),
                      ("TUNER_DUAL_AVERAGING", L.TUNER_DUAL_AVERAGING), ("TUNE_POOLED", L.TUNE_POOLED)):
        assert re.search(name + r"[^\n]*Int32\(" + str(val) + r"\)", jl), name
    assert "MON_ACCEPT, MON_HISTORY, MON_SUMMARIES, MON_HIST_LT, MON_HIST_GRAD, MON_HIST_LLLP = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20" in jl


def test_integration_md_links_the_julia_module():
    """INTEGRATION.md links the module and its package test instead of printing them a second time."""
    md = (ROOT / "INTEGRATION.md").read_text()
    assert "(julia/KlaraHIP/src/KlaraHIP.jl)" in md and "(julia/KlaraHIP/test/runtests.jl)" in md
    assert "module KlaraHIP" not in md


def _julia_code_tokens(src):
    """Julia source with comments, strings and character / symbol literals blanked (what is left is code structure)."""
    import re
    out, i, n = [], 0, len(src)
    while i < n:
        c = src[i]
        if c == "#":                                   # (no #= =# block comments in the file: asserted by the caller)
            while i < n and src[i] != "\n":
                i += 1
        elif c == '"':
            i += 1
            while i < n and src[i] != '"':
                i += 2 if src[i] == "\\" else 1
            i += 1; out.append(' "" ')
        elif c == "'" and i + 2 < n and src[i + 2] == "'":          # a character literal (the file uses ' for transposes nowhere)
            i += 3; out.append(" 'c' ")
        else:
            out.append(c); i += 1
    return "".join(out)


def test_julia_module_is_structurally_valid_for_0_6_and_later():
    """julia/KlaraHIP/src/KlaraHIP.jl must load next to Klara itself, i.e. on Julia 0.6 (/root/reference/REQUIRE:1) as well as on
    >= 0.7.  No Julia here, so: (1) block openers and `end`s balance, brackets balance and never cross a block boundary; (2) the
    version-dependent constructs (`Void` / `Cvoid` alias, uninitialised arrays, the argument order of `finalizer`) occur ONLY inside
    the `@static if VERSION < v"0.7.0-"` compatibility block; (3) nothing that only one of the two syntaxes accepts is used."""
    import re
    src = JL.read_text()
    assert "#=" not in src and "=#" not in src
    code = _julia_code_tokens(src)
    # (1) blocks: every opener keyword at statement level needs an `end`
    toks = re.findall(r"@static|[A-Za-z_][A-Za-z_0-9!]*|[()\[\]{}]|:+", code)
    depth, stack, brackets = 0, [], []
    openers = {"function", "if", "for", "while", "struct", "module", "let", "begin", "try", "do", "quote", "macro"}
    prev = ""
    for tk in toks:
        if tk in "([{":
            brackets.append((tk, len(stack)))
        elif tk in ")]}":
            assert brackets, "unbalanced closing bracket"
            op, d = brackets.pop()
            assert {"(": ")", "[": "]", "{": "}"}[op] == tk and d == len(stack), "a bracket pair crosses a block boundary"
        elif prev.endswith(":") and prev != "::" and tk in openers | {"end", "type"}:
            pass                                        # a symbol literal such as :function (none expected, but not a block)
        elif tk in openers or (tk == "type" and prev == "abstract"):
            assert not brackets or tk in ("if", "for"), f"block opener {tk} inside brackets"
            if not brackets:
                stack.append(tk)
        elif tk == "end":
            assert not brackets, "`end` inside brackets (indexing with end is not used in this file)"
            assert stack, "`end` without an opener"
            stack.pop()
        prev = tk
    assert not stack and not brackets, (stack, brackets)
    assert toks.count("module") == 1 and code.rstrip().endswith("end")
    # (2) version-dependent constructs are confined to the compatibility block
    a = src.index('@static if VERSION < v"0.7.0-"'); b = src.index("\nend\n", a) + 5
    compat, rest = src[a:b], _julia_code_tokens(src[:a] + src[b:])
    assert "const Cvoid = Void" in compat and "Array{T}(dims...)" in compat and "Array{T}(undef, dims...)" in compat
    assert "finalizer(obj, f)" in compat and "finalizer(f, obj)" in compat
    for banned in (r"\bundef\b", r"\bVoid\b", r"\bfinalizer\(", r"\bNothing\b", r"\bcodeunits\b", r"\bfindfirst\b", r"\bimmutable\b",
                   r"(?<!abstract )\btype\b", r"\bisnothing\b", r"\bcontains\(", r"\bsomething\("):
        assert not re.search(banned, rest), banned
    # (3) 0.6 has no `Array{T}(undef, ...)`, >= 0.7 has no `Array{T}(dims)`: outside the block arrays come from newarray / literals / similar
    assert not re.search(r"\b(Array|Vector|Matrix)\{[^}]*\}\(", rest)
    assert rest.count("newarray(") >= 8 and rest.count("on_finalize(") == 3


def _klara_names():
    """tests/golden/klara_exports.txt: what Klara imports from Base to extend, and what it exports (names only; the reference's own lists,
    written by tests/golden/make_klara_exports.py)."""
    txt = (ROOT / "tests" / "golden" / "klara_exports.txt").read_text().splitlines()
    a, b = txt.index("[import Base]"), txt.index("[export]")
    base, exports = {t for t in txt[a + 1:b] if t}, {t for t in txt[b + 1:] if t}
    assert len(base) > 10 and len(exports) > 100 and {"run", "reset"} <= base
    return base, exports


_JULIA_KEYWORDS = {"using", "import", "export", "function", "end", "for", "in", "if", "else", "elseif", "while", "return", "true", "false", "nothing",
                   "const", "struct", "mutable", "module", "do", "isa", "where", "abstract", "type", "begin", "let", "local", "global", "try", "catch"}
# Base / Base.Test names the snippets use (present in Julia 0.6 and later unless noted)
_JULIA_BASE = {"Dict", "randn", "zeros", "ones", "Float64", "UInt8", "Vector", "Matrix", "Symbol", "Any", "println", "print", "push", "LOAD_PATH", "include",
               "size", "maximum", "abs", "first", "methods", "all", "length", "error", "similar", "Base", "Test", "test", "C_NULL",
               "mean",                       # Base.mean on 0.6 (Klara extends it: src/Klara.jl import Base list); Klara runs on 0.6 only (REQUIRE:1)
               "Klara", "KlaraHIP"}


def _julia_snippet_names(code):
    """(identifiers used, identifiers bound) of a Julia snippet: strings / comments blanked, `:sym` literals, `.field` accesses, keyword-argument
    names (`name=` inside a call) and macro names dropped; bound = assignment targets, tuple destructuring, `for x in`, `x ->`."""
    import re
    code = re.sub(r'"""..*?"""', ' "" ', code, flags=re.S)                            # triple-quoted strings (the C text of closures)
    code = _julia_code_tokens(code)
    code = re.sub(r"@[A-Za-z_]+", " ", code)
    code = re.sub(r"(?<![A-Za-z_0-9:]):[A-Za-z_][A-Za-z_0-9!]*", " ", code)          # symbol literals
    code = re.sub(r"\.[A-Za-z_][A-Za-z_0-9!]*", " ", code)                            # field access / dotted operators' operands stay
    bound = set()
    for line in re.split(r"[;\n]", code):
        m = re.match(r"\s*([A-Za-z_][A-Za-z_0-9, ]*?)\s*=(?!=)", line)               # x = ..., a, b, c = ...
        if m and "(" not in m.group(1):
            bound |= {t.strip() for t in m.group(1).split(",") if t.strip()}
        bound |= set(re.findall(r"\bfor\s+([A-Za-z_][A-Za-z_0-9]*)\s+in\b", line))
        bound |= set(re.findall(r"\b([A-Za-z_][A-Za-z_0-9]*)\s*->", line))
    # keyword arguments: `name=value` after `(`, `,` or `;` inside a call
    code = re.sub(r"([(,;]\s*)[A-Za-z_][A-Za-z_0-9]*\s*=(?!=)", r"\1", code)
    used = set(re.findall(r"(?<![A-Za-z_0-9])[A-Za-z_][A-Za-z_0-9]*!?", code))
    used = {u.rstrip("!") if u.rstrip("!") in ("push",) else u for u in used}
    return used, bound


def test_julia_module_exports_and_extends_klaras_generics():
    """`using Klara, KlaraHIP` followed by the module's own header example must work by construction.  No Julia here, so:
    (1) no reach through the caller's top-level module (`Main.`); Klara is imported by name;
    (2) every function the module defines at top level that Klara exports or that Klara imports from Base to extend (run, reset, show ...:
        /root/reference/src/Klara.jl:9-37,45-244) is named in an `import` statement BEFORE its first definition — so the definition adds a
        method to Klara's / Base's generic instead of creating KlaraHIP.<name> (round 3's defect: reset, output);
    (3) every unqualified name used by the header example, by julia/KlaraHIP/test/runtests.jl and by INTEGRATION.md's Julia snippets is
        exported by the module, exported by Klara, a Base name, a Julia keyword, or bound in the snippet itself;
    (4) every exported name is defined in the module; HIPMCJob <: MCJob (Klara's run(::Vector{<:MCJob}) maps over HIP jobs, jobs.jl:212);
    (5) the package layout: REQUIRE names julia 0.6, Klara and Distributions."""
    import re
    src = JL.read_text()
    code = _julia_code_tokens(src)
    base_ext, klara_exports = _klara_names()
    # (1)
    assert not re.search(r"\bMain\b", code)
    assert re.search(r"^import Klara$", code, re.M)
    # imports, in file order
    imports = {}                                        # name -> offset of the import statement
    for m in re.finditer(r"^import ([A-Za-z.]+): ([^\n]*(?:\n[ \t]+[^\n]*)*)", code, re.M):
        for name in re.split(r"[,\s]+", m.group(2)):
            if name:
                imports.setdefault(name, (m.group(1), m.start()))
    assert imports["run"][0] == "Base" and imports["reset"][0] == "Base" and imports["show"][0] == "Base" and imports["output"][0] == "Klara"
    # (2) top-level definitions: `function name(` or `name(args) =` at column 0
    defs = {}
    for m in re.finditer(r"^(?:function\s+)?([A-Za-z_][A-Za-z_0-9!]*)\((?=[^\n]*\)\s*(?:=(?!=)|$|where|\n))", code, re.M):
        defs.setdefault(m.group(1), m.start())
    for m in re.finditer(r"^function\s+([A-Za-z_][A-Za-z_0-9!]*)\(", code, re.M):
        defs.setdefault(m.group(1), m.start())
    assert {"run", "reset", "output", "show", "chainvalue", "chainmeans", "gather_moments", "pooledmoments", "HIPMCJob"} <= set(defs), set(defs)
    for name, at in defs.items():
        if name in klara_exports or name in base_ext:
            assert name in imports and imports[name][1] < at, f"{name} is defined without importing Klara's / Base's generic first"
            owner = "Base" if name in base_ext else "Klara"
            assert imports[name][0] == owner, (name, imports[name][0], owner)
    # (4) exports
    m = re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", code, re.M)
    exported = {t for t in re.split(r"[,\s]+", m.group(1)) if t}
    types = set(re.findall(r"\b(?:struct|abstract type)\s+([A-Za-z_][A-Za-z_0-9]*)", code))
    for name in exported:
        assert name in defs or name in types, f"exported but not defined: {name}"
    assert not (exported & klara_exports), exported & klara_exports      # nothing that would clash with a name Klara exports
    assert re.search(r"mutable struct HIPMCJob <: MCJob\b", code) and "MCJob" in imports
    assert imports["MCJob"][1] < code.index("mutable struct HIPMCJob")
    # types the constructor dispatches on are Klara's own, imported by name
    for t in ("MH", "MALA", "HMC", "SliceSampler", "VanillaMCTuner", "AcceptanceRateMCTuner", "DualAveragingMCTuner",
              "BasicContMuvParameterState", "BasicContMuvParameterNState", "erf_rate_score", "logistic_rate_score"):
        assert imports[t][0] == "Klara" and t in klara_exports, t
    # (3) the snippets
    header = src[:src.index("module KlaraHIP")]
    a = header.index("#     using Klara, KlaraHIP")
    example = "\n".join(l[1:] for l in header[a:].splitlines() if l.startswith("#     "))
    assert "run(job)" in example and "output(job, 1)" in example and "output(job)" in example and "reset(job)" in example and "acceptance(chain)" in example
    assert "likelihood_model(p, false)" in example and "HIPMCJob(model, MH(ones(2))" in example
    snippets = {"header example": example, "runtests.jl": (ROOT / "julia" / "KlaraHIP" / "test" / "runtests.jl").read_text()}
    md = (ROOT / "INTEGRATION.md").read_text()
    for i, block in enumerate(re.findall(r"```julia\n(.*?)```", md, re.S)):
        if not block.startswith("# KlaraHIP.jl"):
            snippets[f"INTEGRATION.md block {i}"] = block
    assert len(snippets) >= 5
    # placeholders the multi-GPU snippet leaves to the caller (its transport and its per-rank inputs), named as such in the text
    caller_supplied = {"bcast_somehow", "rank", "nranks", "device", "sampler", "mcrange", "X0_of_this_rank", "nchains_local", "seed", "D", "p", "job", "comm"}
    for where, text in snippets.items():
        used, bound = _julia_snippet_names(text)
        unknown = used - exported - klara_exports - _JULIA_BASE - _JULIA_KEYWORDS - bound - base_ext
        if where.startswith("INTEGRATION.md"):
            unknown -= caller_supplied
        unknown = {u for u in unknown if not u[0].isdigit()}
        assert not unknown, (where, sorted(unknown))
    # (5)
    req = (ROOT / "julia" / "KlaraHIP" / "REQUIRE").read_text().split("\n")
    assert req[0] == "julia 0.6" and "Klara" in req and any(r.startswith("Distributions") for r in req)


def test_readme_script_runs_with_two_constructor_swaps():
    """VERDICT r4 missing 3: the reference's README script (/root/reference/README.md:17-59) must run on the device after swapping its two constructors —
    BasicContMuvParameter -> HIPParameter, BasicMCJob -> HIPMCJob — with the log-target closure stated as a device target family (Julia closures cannot
    run on a GPU) and `KlaraHIP` added to the `using` line.  No Julia here, so mechanically:
    (1) the substitution undone on INTEGRATION.md's snippet gives the README's own code lines, line for line (their SHA-256 digests, committed as
        tests/golden/readme_example.json by tests/golden/make_readme_example.py), the closure line aside;
    (2) every name the snippet uses is exported by KlaraHIP, exported by Klara, Base or a keyword;
    (3) the module has what the unchanged lines need: HIPParameter is a MUTABLE subtype of Klara's Parameter{Continuous, Multivariate} with `key`, `index`
        and `states` (likelihood_model(p, false) writes p.index: models/GenericModel.jl:110-113), a keyword constructor taking `logtarget=`, and
        HIPMCJob(model::GenericModel, sampler, mcrange, v0; ...) that takes the parameter out of model.vertices (jobs/BasicMCJob.jl:140-185) and
        replicates a start vector over `nchains`; output(job) defaults to chain 1."""
    import hashlib
    import json
    import re
    md = (ROOT / "INTEGRATION.md").read_text()
    snippet = next(b for b in re.findall(r"```julia\n(.*?)```", md, re.S) if "HIPMCJob(model, sampler, mcrange, v0)" in b)
    code = lambda text: [re.sub(r"\s+", " ", l.split("#")[0]).strip() for l in text.splitlines() if l.split("#")[0].strip()]
    # (1) the README's first example (sampling from an unnormalized normal target) and its reset(job, x) continuation, as digests of its code lines
    readme = json.loads((ROOT / "tests" / "golden" / "readme_example.json").read_text())
    swapped = code(snippet)
    assert len(swapped) == len(readme["sha256"]), (len(swapped), len(readme["sha256"]))
    orig = []
    for i, l2 in enumerate(swapped):
        if i == readme["closure_line"]:
            assert l2 == "plogtarget = GaussDiagTarget(2)", l2          # (the README's `plogtarget(z::Vector{Float64}) = ...` closure)
            orig.append(None)
            continue
        l = "using Klara" if l2 == "using Klara, KlaraHIP" else l2.replace("HIPParameter(", "BasicContMuvParameter(").replace("HIPMCJob(", "BasicMCJob(")
        assert hashlib.sha256(l.encode()).hexdigest() == readme["sha256"][i], (i, l)
        orig.append(l)
    assert "reset(job, [3.2, 9.4])" in orig
    assert "BasicMCJob(model, sampler, mcrange, v0)" in " ".join(l for l in orig if l) and "likelihood_model(p, false)" in " ".join(l for l in orig if l)
    assert sum(a != b for a, b in zip(orig, swapped)) == 4                         # the using line, the closure, the two constructors
    src = JL.read_text()
    jcode = _julia_code_tokens(src)
    base_ext, klara_exports = _klara_names()
    m = re.search(r"^export ([^\n]*(?:\n[ \t]+[^\n]*)*)", jcode, re.M)
    exported = {t for t in re.split(r"[,\s]+", m.group(1)) if t}
    used, bound = _julia_snippet_names(snippet)
    unknown = {u for u in used - exported - klara_exports - _JULIA_BASE - _JULIA_KEYWORDS - bound - base_ext if not u[0].isdigit()}
    assert not unknown, sorted(unknown)
    assert {"likelihood_model", "MH", "BasicMCRange", "output"} <= klara_exports and {"run"} <= base_ext
    # (3)
    body = re.search(r"mutable struct HIPParameter <: Parameter\{Continuous, Multivariate\}\n(.*?)\nend", jcode, re.S).group(1)
    fields = [l.strip().split("::")[0] for l in body.splitlines() if l.strip()]
    assert fields[:2] == ["key", "index"] and "states" in fields and "target" in fields, fields
    assert re.search(r"import Klara:[^\n]*(?:\n[ \t]+[^\n]*)*\bParameter\b", jcode) and re.search(r"import Klara:[^\n]*(?:\n[ \t]+[^\n]*)*\bGenericModel\b", jcode)
    assert re.search(r"^import Distributions: Continuous, Multivariate$", jcode, re.M)
    assert "Parameter" in klara_exports and "GenericModel" in klara_exports and "VariableStateVector" in klara_exports
    assert re.search(r"^HIPParameter\(key::Symbol; logtarget::HIPTarget", jcode, re.M)
    ctor = jcode[jcode.index("function HIPMCJob(model::GenericModel, sampler, mcrange, v0::Dict;"):]
    ctor = ctor[:ctor.index("\nend\n")]
    assert "model.vertices[pindex]" in ctor and "firstparameter(model.vertices)" in ctor and "isa(vs[i], Parameter)" in jcode and "HIPMCJob(parameter, sampler, mcrange, v0; kwargs...)" in ctor
    assert "nchains::Integer=1" in jcode and "startmatrix(v0[parameter.key], nchains)" in jcode
    assert re.search(r"^function output\(job::HIPMCJob, c::Integer=1\)", jcode, re.M)
    assert re.search(r"^reset\(job::HIPMCJob, x::AbstractVector\) =", jcode, re.M) and "reset(job, startmatrix(x, job.nchains))" in jcode


def test_instruction_budgets_follow_from_their_parts():
    """scripts/instruction_budget.py (what bench.py's algorithmic roofline fractions divide by): the totals are the sums of the parts
    profiles/README.md derives, and the building blocks are the operation counts of detmath.h's functions."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("instruction_budget", ROOT / "scripts" / "instruction_budget.py")
    B = importlib.util.module_from_spec(spec); spec.loader.exec_module(B)
    assert (B.PHILOX, B.U52, B.U44, B.LOG_U01, B.SQRT_RAD, B.SINCOS, B.BOX_MULLER, B.NORMAL_PAIR, B.NORMAL_PAIR_OWN) == (41, 4, 4, 23, 11, 18, 59, 79.5, 100)
    assert [B.philox_blocks(n) for n in (1, 8, 9, 16, 17, 50, 64)] == [1, 8, 8, 8, 9, 26, 32]       # pairs p and p + 8 share a block
    assert B.mala_diag_unitw_element() == 18
    h4, h8 = B.BUDGETS["headline_4lane"], B.BUDGETS["headline_8lane"]
    assert h4["per_pair"] == 59 + 2 * 18 and h4["pair_evaluations_per_lane"] == 12.5 and h4["philox_blocks_per_lane"] == 6.5 and h4["chains_per_wave"] == 16
    assert h4["per_wave_transition"] == 12.5 * 95 + 6.5 * 41 + 39 + 9 + 3 == 1505.0                    # (rounds 2-3, a block per pair: 1,776)
    assert h8["per_wave_transition"] == 6.25 * 95 + 3.25 * 41 + 27 + 9 + 3
    c5, c4 = B.BUDGETS["cfg5"], B.BUDGETS["cfg4"]
    assert c5["per_leapfrog"] == 26 + 4 * 21 + 45 + 50 + 13 == 218 and c5["per_wave_transition"] == 7808 and c5["normals"] == 5 * 100 + 14
    # cfg 4 (round 4): 4 lanes per chain, 50 rows per lane; a row = Xp (4) + exp(-|Xp|) (18) + 1 + t (1) + log on [1, 2] (12) + softplus (2) + numerator select (3)
    # + division (8) + Xp y (2) + sum (1) + residual (1) + gradient (4) + row offset (1)
    assert (B.EXP_NEG, B.LOG12, B.DIV_UNIT) == (18, 12, 8)
    assert c4["per_row"] == 4 + 18 + 1 + 12 + 2 + 3 + 8 + 2 + 1 + 1 + 4 + 1 == 57 and c4["rows_per_lane"] == 50 and c4["chains_per_wave"] == 16
    assert c4["per_wave_transition"] == 50 * 57 + 36 + 64 + 112 + 60 + 12 == 3134
    # round 4: budgets for the kernels whose fraction used to be null
    c1, hi, sl, sll = B.BUDGETS["cfg1"], B.BUDGETS["hmc_iso"], B.BUDGETS["slice_d100"], B.BUDGETS["slice_d100_lockstep"]
    assert c1["per_wave_transition"] == 100 + 4 + 5 + 72 + 6 + 13 + 2 == 202 and c1["chains_per_wave"] == 64
    assert hi["per_pair"] == 59 + 8 + 2 + 60 + 4 == 133 and hi["per_wave_transition"] == 6.25 * 137 + 3.25 * 41 + 27 + 46 + 3
    assert sl["per_probe"] == 3 and sl["fixed_per_coordinate"] == 82 and sl["per_shrink_attempt"] == 20 and sl["per_expansion"] == 8 and sl["coordinate_slots_per_lane"] == 12.5
    pc = B.slice_probe_counts()                                   # the seeded simulation of the stepping-out procedure reproduces the constants
    assert np.allclose(pc["per_chain"], B.SLICE_PROBES["per_chain"], rtol=1e-12) and np.allclose(pc["max_over_64_lanes"], B.SLICE_PROBES["max_over_64_lanes"], rtol=1e-12) and np.allclose(pc["shrink_blocks"], B.SLICE_PROBES["shrink_blocks"], rtol=1e-12)
    assert 2.0 < pc["per_chain"][0] < 2.3 and 1.3 < pc["per_chain"][2] < 1.6 and sll["per_wave_slot"] > 1.5 * sl["per_wave_slot"]
    # the README of profiles/ quotes these totals
    txt = (ROOT / "profiles" / "README.md").read_text()
    for v in ("1,505", "7,808", "3,134"):
        assert v in txt, v


def test_julia_stub_binds_only_declared_symbols():
    import re
    jl = JL.read_text()
    names = set(re.findall(r"ccall\(\(:([a-z_0-9]+), lib\)", jl))
    assert names and names <= set(L.EXPORTS), names - set(L.EXPORTS)
    assert {"klara_create", "klara_set_state", "klara_run", "klara_reset", "klara_destroy", "klara_get_chain"} <= names


def test_strerror(klib):
    assert klib.klara_strerror(0) == b"ok"
    assert b"finite" in klib.klara_strerror(L.ERR_NONFINITE_INIT)


def test_create_validates_like_the_reference_constructors(klib):
    def status(**over):
        kw = dict(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(2), nchains=4, nsteps=10)
        kw.update(over)
        try:
            K.Engine(**kw).close()
        except K.KlaraError as e:
            return e.status
        return 0
    # invalid arguments are rejected before any device is touched (MALA.jl:65, HMC.jl:94-95,
    # SliceSampler.jl:27, BasicMCRange.jl:22-24, AcceptanceRateMCTuner.jl:32-33)
    assert status(driftstep=-1.0) == L.ERR_INVALID_ARG
    assert status(sampler=L.SAMPLER_HMC, leapstep=0.0) == L.ERR_INVALID_ARG
    assert status(sampler=L.SAMPLER_HMC, nleaps=0) == L.ERR_INVALID_ARG
    assert status(sampler=L.SAMPLER_SLICE, slice_widths=[1.0, -1.0]) == L.ERR_INVALID_ARG
    assert status(sampler=L.SAMPLER_MH) == L.ERR_INVALID_ARG            # sigma missing
    assert status(nsteps=5, burnin=5) == L.ERR_INVALID_ARG
    assert status(thinning=0) == L.ERR_INVALID_ARG
    assert status(period=0) == L.ERR_INVALID_ARG
    assert status(tuner=L.TUNER_ACCEPT_RATE, targetrate=1.5) == L.ERR_INVALID_ARG
    assert status(nchains=0) == L.ERR_INVALID_ARG
    assert status(target=K.GaussDiagTarget.negdot(1025)) == L.ERR_UNSUPPORTED        # (round 6: 64 lanes per chain serve 513 .. 1024 dimensions)
    # the later additions to the descriptor are validated in the same place
    assert status(bm_batchlen=10) == L.ERR_INVALID_ARG                   # streaming batch means need the running sums
    assert status(bm_batchlen=-1, monitor=L.MON_SUMMARIES) == L.ERR_INVALID_ARG
    assert status(nstreams=5) == L.ERR_INVALID_ARG
    assert status(tuner=L.TUNER_DUAL_AVERAGING, targetrate=0.6, da_nadapt=10) == L.ERR_UNSUPPORTED      # HMC only (HMC.jl:124-133)
    assert status(sampler=L.SAMPLER_HMC, tuner=L.TUNER_DUAL_AVERAGING, targetrate=0.6, da_nadapt=0) == L.ERR_INVALID_ARG
    assert status(sampler=L.SAMPLER_MH, mh_sigma=[1.0, 1.0], monitor=L.MON_HIST_GRAD) in (L.ERR_INVALID_ARG, L.ERR_HIP)
    import cases
    assert status(target=K.CustomTarget(1025, cases.SRC_NEGDOT)) == L.ERR_UNSUPPORTED                  # 64 lanes x 16 elements: D <= 1024 (round 6; 256 before)
    assert status(target=K.CustomTarget(2, cases.SRC_NEGDOT, data=np.zeros(0))) in (0, L.ERR_HIP)       # empty data block is fine
    rng = np.random.default_rng(0)
    big = K.LogisticTarget(rng.standard_normal((3687, 4)), np.zeros(3687))
    assert status(target=big, driftstep=0.01) == L.ERR_UNSUPPORTED                                     # data rows must fit the LDS budget
    assert status(sampler=L.SAMPLER_SLICE, slice_widths=np.ones(8), target=K.GaussDenseTarget(np.eye(8))) in (0, L.ERR_HIP)   # (no device here)
    assert status(sampler=L.SAMPLER_HMC, target=K.GaussDenseTarget(np.eye(257))) in (0, L.ERR_HIP)                            # (round 6: 257 .. 1024 on the workgroup-split layout)
    assert status(sampler=L.SAMPLER_HMC, target=K.GaussDenseTarget(np.eye(1025))) == L.ERR_UNSUPPORTED


def test_no_cpu_fallback_without_gpu(klib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(K.KlaraError) as ei:
        K.Engine(sampler=L.SAMPLER_MALA, target=K.GaussDiagTarget.negdot(2), nchains=4, nsteps=10)
    assert ei.value.status == L.ERR_HIP


def test_bench_and_smoke_refuse_to_run_without_a_gpu():
    """The measured path and the smoke check have no CPU fallback either: both stop with an error on a box without a GPU."""
    import subprocess, sys, torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True, text=True)
    assert r.returncode != 0 and "needs a GPU" in (r.stderr + r.stdout)
    r = subprocess.run([sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"], capture_output=True, text=True, cwd=str(ROOT))
    assert r.returncode != 0 and "KlaraError" in r.stderr


def test_bench_dump_outputs_are_a_fixed_float64_sample_within_the_budget(tmp_path):
    """bench.py --dump-outputs (the array writer, no GPU needed): per-chain arrays of a job larger than the cap are written for a fixed, seeded,
    sorted sample of chains named by `chain_index`, pooled arrays whole, everything float64 and within 64 MB; the same job gives the same files;
    a small job is written whole."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    B = importlib.util.module_from_spec(spec); spec.loader.exec_module(B)
    n, D = 40000, 100
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, D))
    per = {"x": x, "logtarget": -(x ** 2).sum(axis=1), "accept_count": rng.integers(0, 9, n).astype(np.uint64), "chain_sum": 3.0 * x, "chain_sumsq": x * x}
    pooled = {"summary_mean": x.mean(axis=0), "summary_counts": [7, 3, n * 25]}
    names = B.dump_outputs(tmp_path / "a", per, pooled, 1000 + np.arange(n))
    assert names == sorted(["chain_index", "x", "logtarget", "accept_count", "chain_sum", "chain_sumsq", "summary_mean", "summary_counts"])
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in names}
    assert all(v.dtype == np.float64 for v in a.values()) and sum((tmp_path / "a" / f"{k}.npy").stat().st_size for k in names) <= 64 * 10 ** 6
    rows = a["chain_index"].astype(np.int64) - 1000
    assert len(rows) == B.DUMP_MAX_CHAINS and np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    for k in per:
        assert np.array_equal(a[k], np.asarray(per[k], dtype=np.float64)[rows]), k
    assert np.array_equal(a["summary_mean"], x.mean(axis=0)) and list(a["summary_counts"]) == [7.0, 3.0, n * 25.0]
    B.dump_outputs(tmp_path / "b", per, pooled, 1000 + np.arange(n))
    assert all(np.array_equal(a[k], np.load(tmp_path / "b" / f"{k}.npy")) for k in names)
    # a job within the cap: every chain, in order
    B.dump_outputs(tmp_path / "c", {"x": x[:100]}, {}, np.arange(100))
    assert np.array_equal(np.load(tmp_path / "c" / "x.npy"), x[:100]) and np.array_equal(np.load(tmp_path / "c" / "chain_index.npy"), np.arange(100.0))
    # per-chain rows wider than the cap allows: fewer chains, still within the budget
    B.dump_outputs(tmp_path / "d", {"x": np.zeros((20000, 1000))}, {}, np.arange(20000))
    assert sum(p.stat().st_size for p in (tmp_path / "d").glob("*.npy")) <= 64 * 10 ** 6


def test_committed_bench_lines_are_complete_and_recomputable():
    """profiles/r2_bench_*.json are the JSON lines bench.py printed on the GPU box: the driver's keys, a roofline whose fraction can be
    recomputed from the committed PMC summary (SQ_ACTIVE_INST_VALU x 4 / 1,024 SIMDs / (launch duration x 2.4 GHz)) and does not exceed 1,
    the HBM side with traffic >= the minimum, a {bound, frac} object for every other configuration, and the CPU baseline."""
    import json
    pmc = json.loads((ROOT / "profiles" / "r2_pmc_kernels.json").read_text())
    rows = {(r["kernel"], r.get("grid")): r["counters"] for r in pmc["kernels"]}
    for name in ("r2_bench_default.json", "r2_bench_driver_flags.json"):
        d = json.loads((ROOT / "profiles" / name).read_text())
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
            assert k in d, (name, k)
        assert d["n_gpus"] == 1 and d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"] == "synthetic" and d["unit"] == "transitions/s"
        assert d["value"] == pytest.approx(d["config"]["nchains_total"] * d["steps"] / (d["ms_per_step"] * d["steps"] * 1e-3), rel=1e-9)
        rf = d["roofline"]
        assert rf["bound"] == "valu" and 0.5 < rf["frac"] <= 1.0
        c = next(v for (kn, g), v in rows.items() if kn == rf["pmc_kernel"] and g == 262144)
        assert rf["frac"] == pytest.approx(4.0 * c["SQ_ACTIVE_INST_VALU"]["mean"] / 1024 / (rf["launch_us"] * 1e-6 * 2.4e9), rel=1e-6)
        h = rf["hbm"]
        assert h["traffic_bytes_per_launch"] >= h["minimal_bytes_per_launch"] and h["traffic_over_minimal"] < 1.25 and h["traffic_frac_of_8TBs"] < 0.1
        ex = d["extra"]
        for key in ("cfg1_roofline", "cfg3_hmc_dense_roofline", "cfg4_roofline", "cfg5_roofline", "hmc_iso_roofline", "slice_d100_roofline",
                    "mala_one_transition_per_launch_roofline"):
            assert ex[key]["bound"] in ("valu", "mfma") and ex[key]["frac"] is not None and 0.3 < ex[key]["frac"] <= 1.0, (name, key, ex[key])
        assert ex["cfg3_hmc_dense_leapfrog_chain_per_s"] >= 1e8                       # north_star's HMC target
        cb = d["cpu_baseline"]
        assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and d["value"] / cb["value"] > 10


def test_round5_bench_lines_are_complete_and_recomputable():
    """profiles/r5_bench_{default,driver_flags}.json, the JSON lines bench.py printed on the closing box: the driver's keys; the headline fraction recomputed from
    the committed budget and the line's own launch duration, its VALU-busy figure from the committed counters (profiles/r5_pmc_kernels.json), rocprofv3's average of
    the same kernel (profiles/r5_bench_headline_kernel_stats.csv) within 6 % of the HIP-event duration; every other configuration's roofline object; the slice
    sampler's counters (frac >= 0.45, SALU / VALU <= 0.3, >= 9e10 coordinate updates/s); cfg 3 at >= 0.88 of the MFMA peak with 0 B scratch."""
    import csv, json
    pmc = json.loads((ROOT / "profiles" / "r5_pmc_kernels.json").read_text())
    stats = {r["Name"]: r for r in csv.DictReader((ROOT / "profiles" / "r5_bench_headline_kernel_stats.csv").open())}
    head_avg_us = float(next(v for k, v in stats.items() if k.startswith("void k_diagt<1, 13, 4, false, true, true,"))["AverageNs"]) * 1e-3
    for name in ("r5_bench_default.json", "r5_bench_driver_flags.json"):
        d = json.loads((ROOT / "profiles" / name).read_text())
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
            assert k in d, (name, k)
        assert d["n_gpus"] == 1 and d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"] == "synthetic" and d["unit"] == "transitions/s"
        assert "configs[1]" in d["config"]["workload"] and d["config"]["save_rule"].startswith("running sums")
        assert d["value"] == pytest.approx(d["config"]["nchains_total"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
        rf = d["roofline"]
        assert rf["bound"] == "valu" and rf["budget"]["per_wave_transition"] == 1505.0
        nec = 1505.0 * 4096 * 32
        assert rf["necessary_valu_insts_per_launch"] == nec
        assert rf["frac"] == pytest.approx(4.0 * nec / (rf["launch_us"] * 1e-6) / (1024 * 2.4e9), rel=1e-9) and 0.65 < rf["frac"] < 1.0
        assert abs(rf["launch_us"] / head_avg_us - 1.0) < 0.06, (rf["launch_us"], head_avg_us)      # (two processes on one box: clocks differ by a few per cent run to run)
        row = next(r for r in pmc["kernels"] if r["kernel"] == rf["pmc"]["kernel"] and r.get("grid") == 262144)
        assert rf["pmc"]["stale"] is False
        assert rf["utilisation"] == pytest.approx(4.0 * row["counters"]["SQ_ACTIVE_INST_VALU"]["mean"] / (rf["launch_us"] * 1e-6) / (1024 * 2.4e9), rel=1e-6)
        assert rf["issued_over_necessary"] == pytest.approx(row["counters"]["SQ_INSTS_VALU"]["mean"] / nec, rel=1e-9) and rf["issued_over_necessary"] < 1.12
        h = rf["hbm"]
        assert h["contract_2S_plus_1_bytes_per_launch"] == 65536 * 3217 and h["traffic_over_minimal"] < 1.25 and h["traffic_frac_of_8TBs"] < 0.1
        ex = d["extra"]
        for key in ("cfg1_roofline", "cfg3_hmc_dense_roofline", "cfg4_roofline", "cfg5_roofline", "hmc_iso_roofline", "slice_d100_roofline", "mala_one_transition_per_launch_roofline"):
            assert ex[key]["bound"] in ("valu", "mfma") and ex[key]["frac"] is not None and 0.3 < ex[key]["frac"] <= 1.0, (name, key, ex[key])
        sl = ex["slice_d100_roofline"]
        assert "k_diagt_slice_free<8, true, false, 1>" in sl["pmc"]["kernel"] and sl["pmc"]["stale"] is False and sl["pmc"]["loaded_scratch"] == 0
        srow = next(r for r in pmc["kernels"] if r["kernel"] == sl["pmc"]["kernel"])
        assert sl["frac"] >= 0.45 and sl["utilisation"] > 0.9 and sl["issued_over_necessary"] < 2.0
        assert srow["counters"]["SQ_INSTS_SALU"]["mean"] / srow["counters"]["SQ_INSTS_VALU"]["mean"] < 0.3
        assert ex["slice_d100_coordinate_updates_per_s"] >= 9e10
        c3 = ex["cfg3_hmc_dense_roofline"]
        assert c3["frac"] >= 0.88 and c3["pmc"]["loaded_scratch"] == 0 and "k_dense_transitions<2, 25, false, false, true>" in c3["pmc"]["kernel"]
        assert ex["cfg3_hmc_dense_leapfrog_chain_per_s"] >= 1e8 and ex["hmc_iso_leapfrog_chain_per_s"] >= 1e8          # north_star's HMC target
        cb = d["cpu_baseline"]
        assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb


def test_round6_bench_lines_are_complete_and_recomputable():
    """profiles/r6_bench_{default,driver_flags}.json (the round's profile pass: one box for the counters, one for the lines): the driver's keys with `roofline.traffic` among
    the first; the headline fraction from the UNCHANGED 1,505-instruction budget and the line's own launch duration, rocprofv3's average of the same kernel within 6 %; the
    fraction over the timed region; the collective the line names; the mixing-step, general-target slice, matrix-core logistic and split-dense extras; cfg 3 at >= 0.88 of the MFMA peak."""
    import csv, json
    pmc = json.loads((ROOT / "profiles" / "r6_pmc_kernels.json").read_text())
    stats = {r["Name"]: r for r in csv.DictReader((ROOT / "profiles" / "r6_bench_headline_kernel_stats.csv").open())}
    head_avg_us = float(next(v for k, v in stats.items() if k.startswith("void k_diagt<1, 13, 4, false, true, true,"))["AverageNs"]) * 1e-3
    for name in ("r6_bench_default.json", "r6_bench_driver_flags.json"):
        d = json.loads((ROOT / "profiles" / name).read_text())
        for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
            assert k in d, (name, k)
        assert d["n_gpus"] == 1 and d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"] == "synthetic" and d["unit"] == "transitions/s"
        assert d["value"] == pytest.approx(d["config"]["nchains_total"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
        col = d["config"]["collective"]
        assert col["requested"] == "klara" and col["used"].startswith("none") and col["error"] is None and d["config"]["rccl_ranks_seen"] == 1
        rf = d["roofline"]
        assert list(rf)[:6] == ["bound", "achieved", "peak", "unit", "frac", "traffic"]                 # (the driver's parse keeps the first scalar keys)
        assert rf["bound"] == "valu" and rf["budget"]["per_wave_transition"] == 1505.0 and rf["traffic"] > 1e8
        nec = 1505.0 * 4096 * 32
        assert rf["necessary_valu_insts_per_launch"] == nec
        assert rf["frac"] == pytest.approx(4.0 * nec / (rf["launch_us"] * 1e-6) / (1024 * 2.4e9), rel=1e-9) and 0.65 < rf["frac"] < 1.0
        assert abs(rf["launch_us"] / head_avg_us - 1.0) < 0.06, (rf["launch_us"], head_avg_us)
        assert rf["frac_timed_region"] == pytest.approx(4.0 * 1505.0 * 4096 / (d["config"]["timed_region_kernel_ms_per_step"] * 1e-3) / (1024 * 2.4e9), rel=1e-9)
        row = next(r for r in pmc["kernels"] if r["kernel"] == rf["pmc"]["kernel"] and r.get("grid") == 262144)
        assert rf["pmc"]["stale"] is False and rf["pmc"]["file"] == "profiles/r6_pmc_kernels.json"
        assert rf["utilisation"] == pytest.approx(4.0 * row["counters"]["SQ_ACTIVE_INST_VALU"]["mean"] / (rf["launch_us"] * 1e-6) / (1024 * 2.4e9), rel=1e-6)
        assert rf["issued_over_necessary"] == pytest.approx(row["counters"]["SQ_INSTS_VALU"]["mean"] / nec, rel=1e-9) and rf["issued_over_necessary"] < 1.12
        ex = d["extra"]
        for key in ("cfg1_roofline", "cfg3_hmc_dense_roofline", "cfg4_roofline", "cfg5_roofline", "hmc_iso_roofline", "slice_d100_roofline", "mala_one_transition_per_launch_roofline",
                    "mala_d100_mixing_step_roofline", "logistic_d64_n200_hmc_L10_roofline"):
            assert ex[key]["bound"] in ("valu", "mfma") and ex[key]["frac"] is not None and 0.3 < ex[key]["frac"] <= 1.0, (name, key, ex[key])
        assert 0.5 < ex["mala_d100_mixing_step"]["acceptance_rate"] < 0.62 and ex["mala_d100_mixing_step_transitions_per_s"] > 3e9
        assert ex["logistic_d64_n200_mala_transitions_per_s"] > 3e8 and ex["logistic_d64_n200_mala_roofline"]["layout"] == [5, 4, 16]       # (closure form: 4.7e7)
        assert ex["slice_swiss_logistic_coordinate_updates_per_s"] > 3e8
        assert ex["slice_pair_closure_d100_coordinate_updates_per_s"] > 3e10 and ex["slice_pair_closure_d100_layout"][0] == 3       # (round 6: the few-lanes kernels; the whole-vector form ran at 7.4e8)
        # dense targets beyond D = 256 on the workgroup-split layout (round 6; refused before): HMC >= 0.8 of the FP64-MFMA peak, MALA >= 0.55
        for dd, lo_h, lo_m in ((512, 0.84, 0.58), (1024, 0.86, 0.68)):
            assert ex[f"hmc_dense_d{dd}_roofline"]["frac"] >= lo_h and ex[f"mala_dense_d{dd}_roofline"]["frac"] >= lo_m, dd
            assert "layout kind 6" in ex[f"hmc_dense_d{dd}_roofline"]["kernel"]
        c3 = ex["cfg3_hmc_dense_roofline"]
        assert c3["frac"] >= 0.88 and c3["pmc"]["loaded_scratch"] == 0
        assert ex["cfg3_hmc_dense_leapfrog_chain_per_s"] >= 1e8 and ex["hmc_iso_leapfrog_chain_per_s"] >= 1e8          # north_star's HMC target
        assert ex["slice_d100_coordinate_updates_per_s"] >= 1.0e11
        cb = d["cpu_baseline"]
        assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    d = json.loads((ROOT / "profiles" / "r6_bench_default.json").read_text())
    assert d["roofline"]["frac_timed_region"] > d["roofline"]["frac"] and d["roofline"]["frac_timed_region"] > 0.76


def test_slice_and_dense_kernel_resources(tmp_path):
    """No GPU needed: the free-running slice kernels (one machine per lane) fit 8 / 6 wavefronts per SIMD without scratch, and the cfg 3 kernel
    (k_dense_transitions<HMC, NE = 25, PLAIN>) has no scratch (round 4: 64-80 B)."""
    import re, shutil, subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    meta = {}
    for tu in ("klara_diagt_slice", "klara_dense"):
        out = tmp_path / f"{tu}.s"
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "klara.jl_amd" / "csrc"),
                            "-S", "--cuda-device-only", "-o", str(out), str(ROOT / "klara.jl_amd" / "csrc" / f"{tu}.hip")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        for blk in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", out.read_text(), re.S):
            t = blk.group(0)
            meta[re.search(r"\.name:\s+(\S+)", t).group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", t).group(1)) for k in ("vgpr_count", "private_segment_fixed_size")}
    free = {k: v for k, v in meta.items() if k.startswith("_Z18k_diagt_slice_freeILi8E") and k.split("EEv")[0].endswith("ELi1")}
    assert len(free) == 4, sorted(free)
    for k, v in free.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_count"] <= (64 if "ILi8ELb1ELb0ELi1" in k else 80), (k, v)
    plain = [v for k, v in meta.items() if k.startswith("_Z19k_dense_transitionsILi2ELi25ELb0E") and k.split("EEv")[0].endswith("Lb1")]
    assert len(plain) == 2 and all(v["private_segment_fixed_size"] == 0 for v in plain), plain


def test_basic_mc_range():
    r = K.BasicMCRange(nsteps=10000, burnin=1000)
    assert (r.nsteps, r.burnin, r.thinning, r.npoststeps) == (10000, 1000, 1, 9000)
    r = K.BasicMCRange(nsteps=100, burnin=10, thinning=7)     # StepRange normalises last: 11:7:100 -> last 95
    assert list(r.postrange)[:2] == [11, 18] and r.nsteps == 95 and r.npoststeps == 13
    for bad in (dict(nsteps=5, burnin=5), dict(burnin=-1), dict(thinning=0)):
        with pytest.raises(AssertionError):
            K.BasicMCRange(**bad)


def test_sampler_and_tuner_constructors():
    assert (K.HMC().leapstep, K.HMC().nleaps) == (0.1, 10)             # HMC.jl:100
    assert K.MALA().driftstep == 1.0                                   # MALA.jl:70
    assert (K.VanillaMCTuner().period, K.VanillaMCTuner().verbose) == (100, False)   # test/VanillaMCTuner.jl:6-9
    t = K.AcceptanceRateMCTuner(0.234)
    assert (t.period, t.verbose) == (100, False)                       # test/AcceptanceRateMCTuner.jl:21-23
    assert list(K.SliceSampler(1.0, 5).widths) == [1.0] * 5            # test/SliceSampler.jl:13
    for ctor in (lambda: K.MALA(0.0), lambda: K.HMC(-0.1), lambda: K.HMC(0.1, 0), lambda: K.SliceSampler([1.0, 0.0]),
                 lambda: K.AcceptanceRateMCTuner(1.0), lambda: K.VanillaMCTuner(0)):
        with pytest.raises(AssertionError):
            ctor()
    assert K.logistic(0.7, 3, 4, 2.1, 1.4) == pytest.approx(1.4110527196983078, rel=1e-15)
    assert K.logistic_rate_score(0.25) == pytest.approx(1.7039056039366212, rel=1e-15)


def test_jobs_built_without_a_seed_get_distinct_streams():
    """two jobs built with default arguments must not share their random stream (the reference's jobs draw from one
    global generator, so `run([job1, job2])` gives independent chains).  The default key is fresh per job; an explicit seed is kept."""
    from klara_jl_amd import api
    a, b, c = api._next_job_seed(), api._next_job_seed(), api._next_job_seed()
    assert len({a, b, c}) == 3 and all(0 <= v < 2 ** 64 for v in (a, b, c))
    # reset(job) moves a job to seed + k * KLARA_EPOCH_KEY_STRIDE; no default key of a later job may sit on that
    # progression (job i after k resets must not replay job i + k): the default keys are hashed, not equally spaced
    stride = 0x9E3779B97F4A7C15
    keys = [api._next_job_seed() for _ in range(64)]
    reset_keys = {(keys[i] + k * stride) % 2 ** 64 for i in range(64) for k in range(1, 65)}
    assert not (reset_keys & set(keys))
    assert api._splitmix64(0) == 0xE220A8397B1DCDAF and api._splitmix64(1) == 0x910A2DEC89025CC1      # Vigna's reference values
    import inspect
    assert inspect.signature(api.BasicMCJob.__init__).parameters["seed"].default is None


def test_target_families():
    t = K.GaussDiagTarget.mvnormal([6.11, -8.5], 1.0)
    assert t.ndims == 2 and np.allclose(t.w, 0.5) and t.const == pytest.approx(-np.log(2 * np.pi))
    p = K.GaussDenseTarget.compound_symmetric(6, 0.5).precision
    sigma = 0.5 * np.eye(6) + 0.5 * np.ones((6, 6))
    assert np.allclose(p @ sigma, np.eye(6))
    with pytest.raises(ValueError):
        K.GaussDenseTarget(np.zeros((2, 3)))
    with pytest.raises(TypeError):
        K.BasicContMuvParameter("p", logtarget=lambda z: -z @ z)       # arbitrary closures cannot run on device


def test_iostream_csv_format(tmp_path):
    """One comma-joined line per saved step with Julia's float printing
    (BasicContParamIOStream.jl:152-159: `join(getfield(state, field), ',')`)."""
    from klara_jl_amd.iostream import julia_float_repr as j, write_chain
    known = {5.1: "5.1", -0.9: "-0.9", 1e-5: "1.0e-5", 0.0001: "0.0001", 1e6: "1.0e6", 123456.0: "123456.0",
             1234567.0: "1.234567e6", 0.1 + 0.2: "0.30000000000000004", 1e22: "1.0e22", 100.0: "100.0",
             1.5e-7: "1.5e-7", -2.5e-10: "-2.5e-10", 1.0: "1.0", 0.0: "0.0", float("inf"): "Inf", float("nan"): "NaN"}
    for x, s in known.items():
        assert j(x) == s, (x, j(x), s)
    rng = np.random.default_rng(0)
    for x in np.concatenate([rng.standard_normal(200), np.exp(rng.uniform(-30, 30, 200))]):
        assert float(j(x)) == x                                   # round-trips
    v = np.array([[5.1, 1e-5], [-0.9, 2.0]])                      # (D=2, n=2): columns are saved steps
    write_chain(str(tmp_path), "csv", v, np.array([-1.5, 2e7]), None, np.array([1, 0], dtype=np.uint8))
    assert (tmp_path / "value.csv").read_text() == "5.1,-0.9\n1.0e-5,2.0\n"
    assert (tmp_path / "logtarget.csv").read_text() == "-1.5\n2.0e7\n"
    assert (tmp_path / "diagnosticvalues.csv").read_text() == "true\nfalse\n"
    assert not (tmp_path / "gradlogtarget.csv").exists()


def test_shard_chains_is_a_partition():
    for n, w in ((65536, 8), (10, 4), (7, 8), (262144, 8)):
        parts = [K.shard_chains(n, r, w) for r in range(w)]
        assert parts[0][0] == 0 and sum(c for _, c in parts) == n
        for (o1, c1), (o2, _) in zip(parts, parts[1:]):
            assert o1 + c1 == o2


def test_custom_target_source_compiles_without_a_gpu():
    """klara_check_custom_target: the user's closures are compiled for gfx950 exactly as klara_create would (hiprtc needs no
    device), so a source error is reported with the user's own line numbers before a job is ever submitted."""
    import cases
    for sampler, d, src in ((L.SAMPLER_MALA, 3, cases.SRC_NEGDOT), (L.SAMPLER_HMC, 32, cases.SRC_QUARTIC_CHAIN),
                            (L.SAMPLER_MH, 2, cases.SRC_BANANA_LT_ONLY), (L.SAMPLER_SLICE, 4, cases.SRC_LOGIT)):
        K.CustomTarget(d, src).check(sampler)
    with pytest.raises(K.KlaraError) as ei:
        K.CustomTarget(2, "KLARA_USER_FN double klara_user_logtarget(const double* x, int D, const double* data, long long n)\n{\n    return x[0] +;\n}").check(L.SAMPLER_MH)
    assert ei.value.status == L.ERR_COMPILE and "klara_user_target:3" in ei.value.log
    with pytest.raises(K.KlaraError) as ei:               # MALA / HMC need the gradient closure
        K.CustomTarget(2, cases.SRC_BANANA_LT_ONLY).check(L.SAMPLER_HMC)
    assert ei.value.status == L.ERR_COMPILE and "klara_user_gradlogtarget" in ei.value.log
    with pytest.raises(K.KlaraError) as ei:
        K.CustomTarget(1025, cases.SRC_NEGDOT).check(L.SAMPLER_MH)
    assert ei.value.status == L.ERR_UNSUPPORTED


def test_pair_closure_jobs_the_pair_kernels_do_not_serve_compile_as_whole_vector_closures():
    """A pair closure below 17 dimensions, or with the slice sampler, used to be refused (KLARA_ERR_UNSUPPORTED); now the library sums the pairs' terms itself
    (klara_custom_compose.h) and compiles the whole-vector form — and the CPU oracle's harness composes the same text, so both sides add the terms pair 0 first."""
    import cases, oracle_ffi as O
    for sampler, d, src, data in ((L.SAMPLER_MALA, 9, cases.SRC_PAIR_QUARTIC, [0.1, 0.4]), (L.SAMPLER_HMC, 16, cases.SRC_PAIR_BANANA, [0.05, 9.0]),
                                  (L.SAMPLER_SLICE, 40, cases.SRC_PAIR_INDEXED, list(np.linspace(0.5, 2.0, 40))), (L.SAMPLER_SLICE, 6, cases.SRC_PAIR_NEGDOT, None),
                                  (L.SAMPLER_MH, 100, cases.SRC_PAIR_NEGDOT, None)):          # (the last one: still the pair-transposed kernels)
        K.CustomTarget.pairwise(d, src, data).check(sampler)
    # the composed closure on the host: the sum of the pairs' terms in ascending pair order, the gradient element by element
    t = K.CustomTarget.pairwise(9, cases.SRC_PAIR_QUARTIC, [0.1, 0.4])
    _, lt, grad, pair = O.compile_user_target("#define KLARA_PAIR_AS_WHOLE 1\n" + t.source, 9)
    assert pair is None and lt is not None and grad is not None
    _, lt2, _, pair2 = O.compile_user_target(t.source, 9)
    assert pair2 is not None and lt2 is None
    x = np.random.default_rng(5).standard_normal(9); dat = np.array([0.1, 0.4])
    f_lt = C.CFUNCTYPE(C.c_double, C.c_void_p, C.c_int, C.c_void_p, C.c_longlong)(lt.value)
    f_pair = C.CFUNCTYPE(C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.POINTER(C.c_double), C.POINTER(C.c_double))(pair2.value)
    s = 0.0
    for P in range(5):
        g0, g1 = C.c_double(), C.c_double()
        s = s + f_pair(x[2 * P], x[2 * P + 1] if 2 * P + 1 < 9 else 0.0, P, 9, dat.ctypes.data, 2, C.byref(g0), C.byref(g1))
    assert f_lt(x.ctypes.data, 9, dat.ctypes.data, 2) == s


def test_custom_target_disk_cache(tmp_path):
    """Run-time compiled code objects are cached on disk (KLARA_JIT_CACHE_DIR): a second process finds the entry instead of
    compiling, a damaged entry is ignored and replaced, KLARA_JIT_CACHE=0 writes nothing."""
    import os, subprocess, sys, time
    code = ("import sys, time; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import cases, klara_jl_amd as K\nfrom klara_jl_amd import _lib as L\n"
            "t0 = time.time(); K.CustomTarget(24, cases.SRC_QUARTIC_CHAIN).check(L.SAMPLER_HMC); print(time.time() - t0)\n"
            % (str(ROOT), str(ROOT / "tests")))
    def run(**env):
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env={**os.environ, **env})
        assert r.returncode == 0, r.stderr
        return float(r.stdout.strip().splitlines()[-1])
    cache = tmp_path / "jit"
    t_cold = run(KLARA_JIT_CACHE_DIR=str(cache))
    files = list(cache.glob("*.kjit"))
    assert len(files) == 1 and files[0].stat().st_size > 10000
    t_warm = run(KLARA_JIT_CACHE_DIR=str(cache))
    assert t_warm < 0.5 * t_cold, (t_cold, t_warm)
    blob = bytearray(files[0].read_bytes()); blob[len(blob) // 2] ^= 0xFF; files[0].write_bytes(bytes(blob))
    run(KLARA_JIT_CACHE_DIR=str(cache))                      # checksum mismatch -> recompiled and rewritten
    assert files[0].read_bytes() != bytes(blob)
    off = tmp_path / "off"
    run(KLARA_JIT_CACHE_DIR=str(off), KLARA_JIT_CACHE="0")
    assert not off.exists() or not list(off.glob("*.kjit"))


def _plan(klib, runs, **kw):
    d = L.KlaraDesc()
    d.struct_size = C.sizeof(L.KlaraDesc); d.abi_version = L.KLARA_ABI_VERSION
    d.sampler, d.target, d.nchains, d.ndims = L.SAMPLER_MALA, L.TARGET_GAUSS_DIAG, 8, 3
    d.driftstep, d.period, d.thinning, d.nsteps = 0.5, 100, 1, sum(runs)
    for key, v in kw.items():
        setattr(d, key, v)
    runs_a = np.asarray(runs, np.int64)
    cap = int(sum(runs)) + 8
    k = np.zeros(cap, np.int64); col = np.zeros(cap, np.int64); ph = np.zeros(cap, np.int32); fl = np.zeros(cap, np.int32)
    n = C.c_int64(0)
    L.check(klib.klara_selftest_plan(C.byref(d), len(runs), runs_a.ctypes.data, cap, k.ctypes.data, col.ctypes.data, ph.ctypes.data,
                                     fl.ctypes.data, C.byref(n)), "selftest_plan")
    n = int(n.value)
    return k[:n], col[:n], ph[:n], fl[:n]


def test_monitors_a_job_cannot_have_are_refused_without_a_device(klib):
    """The gradient history on a sampler that carries no gradient (MH, slice) and the likelihood / prior history on a target that is not a
    likelihood + prior user target are descriptor errors: validate() refuses them (klara_selftest_plan runs it and needs no device), before
    klara_create allocates anything."""
    ones = np.ones(3)
    ptr = ones.ctypes.data_as(C.POINTER(C.c_double))
    _plan(klib, [10], monitor=L.MON_HIST_GRAD)                       # MALA carries one
    for kw in (dict(sampler=L.SAMPLER_MH, mh_sigma=ptr, monitor=L.MON_HIST_GRAD),
               dict(sampler=L.SAMPLER_SLICE, slice_widths=ptr, monitor=L.MON_HIST_GRAD),
               dict(monitor=L.MON_HIST_LLLP)):
        with pytest.raises(K.KlaraError) as e:
            _plan(klib, [10], **kw)
        assert e.value.status == L.ERR_INVALID_ARG, kw


@pytest.mark.parametrize("seed", range(40))
def test_launch_planning_is_pure_host_logic(klib, seed):
    """klara_run's launch splitting, checked without a device against a step-by-step model: every launch stays within
    steps_per_launch, never wraps around the history ring, never crosses an event of the pooled tuner (tuners.jl:27-32: every `period` proposals while
    totproposed <= burnin, totproposed starting at period) or a batch boundary of the streaming batch means, and carries the
    save-rule bookkeeping of BasicMCRange.jl:36 ((burnin+1):thinning:nsteps)."""
    rng = np.random.default_rng(seed)
    burnin, thinning, period = int(rng.choice([0, 5, 30, 100])), int(rng.choice([1, 2, 7])), int(rng.choice([3, 10, 25]))
    spl = int(rng.choice([0, 1, 4, 16, 50]))
    pooled = bool(rng.integers(0, 2)); bm = int(rng.choice([0, 0, 3, 10]))
    ring = int(rng.choice([0, 0, 4, 9, 32])); acov = int(rng.choice([0, 0, 5]))
    runs = [int(v) for v in rng.integers(1, 120, int(rng.integers(1, 5)))]
    total = sum(runs)
    if total <= burnin:
        runs.append(burnin + 1); total = sum(runs)
    kw = dict(burnin=burnin, thinning=thinning, period=period, steps_per_launch=spl, bm_batchlen=bm, hist_ring_cols=ring, acov_maxlag=acov)
    if pooled:
        kw.update(tuner=L.TUNER_ACCEPT_RATE, tuner_mode=L.TUNE_POOLED, targetrate=0.5)
    if bm:
        kw.update(monitor=L.MON_SUMMARIES)
    k, col, ph, fl = _plan(klib, runs, **kw)
    assert k.sum() == total and (k >= 1).all() and (k <= (spl or 32)).all()
    ends = np.cumsum(k); starts = ends - k
    # launches never straddle two klara_run calls
    run_ends = np.cumsum(runs)
    assert set(run_ends) <= set(ends) and np.array_equal(ends[(fl & 4) != 0], run_ends)
    # step-by-step model of the pooled tuner's events and of the batch boundaries
    tune_events, prop, tot = set(), 0, period
    for t in range(1, total + 1):
        prop += 1
        if pooled and tot <= burnin and prop % period == 0:
            tune_events.add(t); tot += prop; prop = 0
    saved = [t for t in range(burnin + 1, total + 1, thinning)]
    batch_ends = {saved[i] for i in range(bm - 1, len(saved), bm)} if bm else set()
    for a, b in zip(starts, ends):
        assert not any(a < e < b for e in tune_events | batch_ends), (a, b)
    assert {int(e) for e, f in zip(ends, fl) if f & 2} == batch_ends
    assert ((fl & 1) != 0).all() == pooled and ((fl & 1) != 0).any() == pooled
    # save rule: columns saved before the launch, and the thinning phase of its first post-burn-in transition; with a history ring
    # (klara_desc.hist_ring_cols, or the 32 columns the streaming autocovariances keep for themselves) the column is the ring slot
    # and no launch wraps around the ring
    rcols = ring if ring else (32 if acov else 0)
    if rcols >= len(saved):
        rcols = 0
    for a, b, c, p_ in zip(starts, ends, col, ph):
        before = len([t for t in saved if t <= a])
        inside = len([t for t in saved if a < t <= b])
        assert c == (before % rcols if rcols else before)
        assert p_ == ((a - burnin) % thinning if a >= burnin else 0)
        if rcols:
            assert c + inside <= rcols, (a, b, c, inside, rcols)


def test_launch_length_follows_the_environment_of_each_planning_call(klib, monkeypatch):
    """A plain slice job on the diagonal Gaussian (D = 100) runs the free-running kernel at KLARA_DEFAULT_STEPS_PER_LAUNCH_SLICE transitions per
    launch, and round 4's lockstep kernel (KLARA_SLICE_LOCKSTEP) at KLARA_DEFAULT_STEPS_PER_LAUNCH.  Every planning call reads the switches
    anew: the first value a process sees is not kept for later jobs."""
    widths = np.ones(100)
    kw = dict(sampler=L.SAMPLER_SLICE, ndims=100, steps_per_launch=0, slice_widths=widths.ctypes.data_as(C.POINTER(C.c_double)))
    lengths = []
    for lockstep in (False, True, False):
        if lockstep:
            monkeypatch.setenv("KLARA_SLICE_LOCKSTEP", "1")
        else:
            monkeypatch.delenv("KLARA_SLICE_LOCKSTEP", raising=False)
        k, _, _, _ = _plan(klib, [256], **kw)
        lengths.append(int(k[0]))
    assert lengths == [L.DEFAULT_STEPS_PER_LAUNCH_SLICE, L.DEFAULT_STEPS_PER_LAUNCH, L.DEFAULT_STEPS_PER_LAUNCH_SLICE]


def _build_c_example(tmp_path):
    import subprocess
    exe = tmp_path / "readme_job"
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O2", "-I", str(ROOT / "include"),
                        str(ROOT / "examples" / "readme_job.c"), "-L", str(ROOT / "klara.jl_amd" / "lib"), "-lklara_hip",
                        f"-Wl,-rpath,{ROOT / 'klara.jl_amd' / 'lib'}", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_header_is_plain_c99_and_the_c_example_links(tmp_path):
    """include/klara_hip.h is a C header (no C++, no torch types): examples/readme_job.c builds with gcc -std=c99 -pedantic
    -Werror against the shared library.  Without a GPU klara_create reports a status code — it never aborts."""
    import subprocess
    exe = _build_c_example(tmp_path)
    import torch
    if not torch.cuda.is_available():
        r = subprocess.run([str(exe), "8"], capture_output=True, text=True)
        assert r.returncode == 1 and "HIP runtime error or no device" in r.stderr


def test_bench_kernel_register_budget(tmp_path):
    """Occupancy guard that needs no GPU: the headline kernel k_diagt<MALA, NP=7, Q=8, ONESTEP, UNITW> must fit 4 wavefronts per
    SIMD (<= 128 VGPRs) without scratch, its fused sibling 3 (<= 168), and the instantiations with the save rule and with the tuner
    bookkeeping 2 (<= 256) — none of them with scratch."""
    import re, shutil, subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    out = tmp_path / "k.s"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "klara.jl_amd" / "csrc"),
                        "-S", "--cuda-device-only", "-o", str(out), str(ROOT / "klara.jl_amd" / "csrc" / "klara_diagt_mala.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = {}
    for blk in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", out.read_text(), re.S):
        t = blk.group(0)
        name = re.search(r"\.name:\s+(\S+)", t).group(1)
        meta[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", t).group(1)) for k in ("vgpr_count", "private_segment_fixed_size")}
    one = next(v for k, v in meta.items() if k.startswith("_Z7k_diagtILi1ELi7ELi8ELb1ELb1ELb0ELb0ELb0E"))
    fused = next(v for k, v in meta.items() if k.startswith("_Z7k_diagtILi1ELi7ELi8ELb0ELb1ELb0ELb0ELb0E"))
    saving = next(v for k, v in meta.items() if k.startswith("_Z7k_diagtILi1ELi7ELi8ELb0ELb1ELb1ELb0ELb0E"))    # + save rule (bench headline)
    tuned = next(v for k, v in meta.items() if k.startswith("_Z7k_diagtILi1ELi7ELi8ELb0ELb1ELb1ELb1ELb0E"))     # + tuner bookkeeping
    assert one["vgpr_count"] <= 128 and one["private_segment_fixed_size"] == 0, one
    assert fused["vgpr_count"] <= 168 and fused["private_segment_fixed_size"] == 0, fused                      # 3 wavefronts per SIMD
    assert saving["vgpr_count"] <= 256 and saving["private_segment_fixed_size"] == 0, saving
    assert tuned["vgpr_count"] <= 256 and tuned["private_segment_fixed_size"] == 0, tuned


def test_streamed_dense_kernels_have_no_register_saves_under_a_partial_mask():
    """scripts/scan_exec_joins.py over klara_dense_big.hip (the 338-512 register kernels: the allocator parks part of their arrays in accumulator
    registers): no block of any kernel saves a register (v_accvgpr_write / scratch_store) between its label and the `s_or_b64 exec` that re-enables
    the other side of a divergent branch — the placement that lost element 15 of every rejecting chain in k_dense_big<MH, 48, mean> before the
    transition loop was made branch-free.  The scanner itself is proven on that pattern."""
    import importlib.util, shutil, subprocess
    spec = importlib.util.spec_from_file_location("scan_exec_joins", ROOT / "scripts" / "scan_exec_joins.py")
    S = importlib.util.module_from_spec(spec); spec.loader.exec_module(S)
    bad = """_Z1kv:
\ts_and_saveexec_b64 s[0:1], s[2:3]
\ts_cbranch_execz .LBB0_2
\tbuffer_load_dwordx2 v[32:33], v4, s[72:75], 0 offen
.LBB0_2:
\ts_waitcnt vmcnt(32)
\tv_accvgpr_write_b32 a53, v33
\tv_accvgpr_write_b32 a52, v32
\ts_or_b64 exec, exec, s[0:1]
\ts_endpgm
"""
    good = bad.replace("\tv_accvgpr_write_b32 a53, v33\n\tv_accvgpr_write_b32 a52, v32\n\ts_or_b64 exec, exec, s[0:1]\n",
                       "\ts_or_b64 exec, exec, s[0:1]\n\tv_accvgpr_write_b32 a53, v33\n\tv_accvgpr_write_b32 a52, v32\n")
    assert [len(v) for v in S.scan(bad).values()] == [1] and [len(v) for v in S.scan(good).values()] == [0]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        out = Path(d) / "k.s"
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-I", str(ROOT / "klara.jl_amd" / "csrc"),
                            "-S", "--cuda-device-only", "-o", str(out), str(ROOT / "klara.jl_amd" / "csrc" / "klara_dense_big.hip")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        hits = S.scan(out.read_text())
    assert len(hits) >= 40                                            # 32 transition kernels + the initialisers
    assert not {k: v for k, v in hits.items() if v}, {k: v[:2] for k, v in hits.items() if v}


def test_iostream_files_round_trip_the_reference_tests_vectors(tmp_path):
    """The :iostream sink's on-disk format against the values the reference's own IO-stream tests write and read back
    (test/ParameterIOStreams.jl:159-193 BasicContMuvParameterState, :195-238 ContMuvMarkovChain; write = one comma-joined line per saved
    state, BasicContParamIOStream.jl:152-159; read = readdlm + transpose, :215-252): the files hold Julia's shortest float printing, and
    `read_chain` returns the matrices / vectors / accept diagnostics exactly."""
    from klara_jl_amd.iostream import ChainWriter, read_chain, julia_float_repr
    # test/ParameterIOStreams.jl:161-163: value and a gradient field of 4 saved states of a 2-vector, their accept diagnostics
    nstatev = np.array([[1.33, 2.44, 3.14, -0.82], [7.21, -9.75, -5.26, -0.63]])
    nstateg = np.array([[3.13, -12.10, 13.11, -0.99], [9.91, -5.25, -8.15, -9.69]])
    nstated = np.array([False, True, True, False])
    w = ChainWriter(str(tmp_path / "a"), "csv", value=True, logtarget=False, gradlogtarget=True, accept=True)
    for i in range(4):                                                   # one write per saved state, as the job loop does (:152-159)
        w.append(value=nstatev[:, i:i + 1], gradlogtarget=nstateg[:, i:i + 1], accept=nstated[i:i + 1])
    w.flush(); w.close()
    assert (tmp_path / "a" / "value.csv").read_text() == "1.33,7.21\n2.44,-9.75\n3.14,-5.26\n-0.82,-0.63\n"          # join(state.value, ',')
    assert (tmp_path / "a" / "gradlogtarget.csv").read_text() == "3.13,9.91\n-12.1,-5.25\n13.11,-8.15\n-0.99,-9.69\n"
    assert (tmp_path / "a" / "diagnosticvalues.csv").read_text() == "false\ntrue\ntrue\nfalse\n"
    assert not (tmp_path / "a" / "logtarget.csv").exists()               # only monitored fields get a file (:64-82)
    c = read_chain(str(tmp_path / "a"))
    assert c.size == 2 and c.n == 4 and np.array_equal(c.value, nstatev) and np.array_equal(c.gradlogtarget, nstateg)
    assert c.diagnostickeys == ["accept"] and np.array_equal(c.diagnosticvalues, nstated[None, :])
    assert c.logtarget.size == 0 and c.loglikelihood.size == 0 and c.logprior.size == 0          # (:for i in [2:4; 6:13] ... length == 0)
    # test/ParameterIOStreams.jl:197-200: value, loglikelihood, logtarget of 3 saved states (the reference uses Float32 there; the values
    # are the decimal literals)
    v2 = np.array([[-1.85, -0.09, 0.36], [-0.45, -0.85, 1.91]]); ll = np.array([-1.30, -1.65, -0.18]); lt = np.array([-0.44, 0.72, -0.21])
    w = ChainWriter(str(tmp_path / "b"), "csv", value=True, logtarget=True, gradlogtarget=False, accept=False, likelihood_prior=True)
    w.append(value=v2, logtarget=lt, loglikelihood=ll, logprior=np.zeros(3)); w.close()
    assert (tmp_path / "b" / "loglikelihood.csv").read_text() == "-1.3\n-1.65\n-0.18\n" and (tmp_path / "b" / "logtarget.csv").read_text() == "-0.44\n0.72\n-0.21\n"
    c = read_chain(str(tmp_path / "b"))
    assert np.array_equal(c.value, v2) and np.array_equal(c.loglikelihood, ll) and np.array_equal(c.logtarget, lt) and c.diagnosticvalues.size == 0
    # the printing round-trips every double (what makes write -> read exact for a real job's values)
    rng = np.random.default_rng(3)
    xs = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-12, 12, 2000), [0.0, -0.0, 1e-5, 1e-4, 999999.0, 1e6, 123456.7, 5e-324, 1.7976931348623157e308]])
    assert all(float(julia_float_repr(x)) == x and np.signbit(float(julia_float_repr(x))) == np.signbit(x) for x in xs)


def test_bench_gpus_n_without_a_launcher_starts_its_own_ranks():
    """VERDICT r3 item 2a, the part that needs no GPU: `python bench.py --gpus 2` with WORLD_SIZE unset re-executes itself under
    torch.distributed.run (one process per rank, 127.0.0.1) instead of exiting with a usage message.  Without a GPU every rank stops at
    "bench.py needs a GPU" — which proves the ranks were started with WORLD_SIZE = 2 — and the launcher's exit code comes back."""
    import os
    import subprocess
    import sys
    import torch
    if torch.cuda.is_available():
        pytest.skip("the GPU form of this test is tests/test_gpu_multi.py::test_bench_starts_its_own_ranks_without_a_launcher")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--backend", "gloo", "--same-device"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=str(ROOT))
    assert r.returncode != 0
    # The launcher line names the rank count it started; at least one rank reaches the GPU check and says which rank of how many it is.  (Not
    # "both ranks": torch.distributed.run sends SIGTERM to the surviving rank as soon as the first one exits, so whether the second message
    # appears is a race — VERDICT r5 weak 3.)
    assert "launch with" not in r.stderr and "--nproc-per-node=2" in r.stderr, r.stderr[-2000:]
    assert r.stderr.count("bench.py needs a GPU") >= 1 and "of 2]" in r.stderr, r.stderr[-2000:]
    # a launcher that started the wrong number of ranks is named as such
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "4"], capture_output=True, text=True, timeout=120,
                       env=dict(env, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), cwd=str(ROOT))
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr
