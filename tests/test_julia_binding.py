"""The Julia binding (waterlily.jl_amd/julia/WaterLilyHIPExt.jl) cannot run here — no Julia exists in this image or on the GPU box.
What can be checked without Julia is checked:
 1. sites.json lists EVERY `@loop` / `@inside` / broadcast / reduction / array-constructor site of the reference files that
    Simulation(...) + sim_step! (+ the force read-outs) reach; this test holds it against the scan of the reference's src/ recorded in
    tests/golden/reference_sites.json (file, line and a hash of the text of every site; tests/golden/make_reference_sites.py makes it)
    and fails on any site that is not listed (or whose line moved); with WATERLILY_JL_SRC naming the reference's src/ directory it
    re-scans the reference and checks the recording first;
 2. every listed site names the method of the binding that intercepts it, and that method's signature is present in the file;
 3. every `ccall` of the binding names a symbol include/wlhip.h declares, with the declared number of arguments;
 4. the Julia mirrors of the C structs (WlGrid, WlBody, WlSimDesc) have the fields of include/wlhip.h in order;
 5. dispatch hazards that only a Julia run would show are desk-checked as text rules (round-2 advisor findings): no method signature
    that is ambiguous with Base's broadcast-style rules, no dictionary keyed by a device array (hashing = scalar getindex per element),
    no per-step path through scalar getindex, the spare velocity array handed over for every flow, uniform closures kept on the composite.
The call SEQUENCE the binding performs for the composite time step is executed, through ctypes, by tests/test_gpu_callerowned.py."""
import hashlib
import json
import os
import re


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JL = os.path.join(ROOT, "waterlily.jl_amd", "julia", "WaterLilyHIPExt.jl")
SITES = os.path.join(ROOT, "waterlily.jl_amd", "julia", "sites.json")
REF_SITES = os.path.join(ROOT, "tests", "golden", "reference_sites.json")
PAT = re.compile(r'@loop|@inside|\.=|\.\*=|\./=|\.\+=|\.-=|\bsum\(|\bmaximum\(|⋅|\bfill!\(|\bcopy\(|\bsimilar\(')
REF_FILES = ("core.jl", "Flow.jl", "Poisson.jl", "MultiLevelPoisson.jl", "Body.jl", "WaterLily.jl", "Metrics.jl")


def text_hash(text):
    return hashlib.sha256(text.encode("utf-8")).hexdigest()[:16]


def scan_reference(src, scope):
    """[file, line, hash of the line's first 110 stripped characters] of every site of the reference's src/ directory, in file order"""
    scope = {k: [tuple(r) for r in v] for k, v in scope.items()}
    found = []
    for f in REF_FILES:
        for i, line in enumerate(open(os.path.join(src, f), encoding="utf-8").read().split("\n"), 1):
            st = line.strip()
            if f in scope and not any(a <= i <= b for a, b in scope[f]):
                continue
            if not PAT.search(line) or st.startswith("#"):
                continue
            found.append(["src/" + f, i, text_hash(st[:110])])
    return found


def test_every_listed_site_has_an_interceptor_in_the_binding():
    src = open(JL, encoding="utf-8").read()
    sites = json.load(open(SITES, encoding="utf-8"))["sites"]
    assert len(sites) > 90
    for s in sites:
        h = s["handled_by"]
        if h is None:
            assert s["how"], s                      # host-only code: the reason is recorded
            continue
        assert h in src, f'{s["file"]}:{s["line"]} is said to be handled by "{h}", which is not in WaterLilyHIPExt.jl'
    # the four broadcast forms of the time-step path go to library calls, not to scalar indexing
    body = re.search(r"function bc_copyto!(.*?)\nend\n", src, re.S).group(1)
    for frag in ("return fill!(dest, x)", "return copyto!(dest, x)", "(:wl_scale, libwlhip)", "(:wl_div_scalar, libwlhip)"):
        assert frag in body, frag
    assert re.search(r"Base\.fill!\(a::HipArray, v\) = .*?\(:wl_fill, libwlhip\)", src) and re.search(r"function Base\.copyto!\(d::HipArray, s::HipArray\).*?\(:wl_d2d, libwlhip\)", src, re.S)
    # the composite the benchmark times has a Julia caller, on the caller's arrays
    for sym in ("wl_sim_create_on", "wl_sim_mom_step", "wl_sim_set_dt_last", "wl_sim_field", "wl_mg_history"):
        assert f"(:{sym}, libwlhip)" in src, sym
    assert "KernelAbstractions.get_backend(::HipArray)" in src and "apply!(f, c::HipArray{T,N})" in src


def test_site_list_is_complete_and_current_against_the_reference():
    j = json.load(open(SITES, encoding="utf-8"))
    rec = json.load(open(REF_SITES, encoding="utf-8"))
    assert rec["pattern"] == PAT.pattern and rec["scope"] == j["scope"], "the recorded scan was made with another pattern or scope"
    src = os.environ.get("WATERLILY_JL_SRC")
    if src:
        assert scan_reference(src, j["scope"]) == rec["sites"], "the reference differs from the recorded scan: rerun tests/golden/make_reference_sites.py"
    listed = {(s["file"], s["line"]): s for s in j["sites"]}
    found = {(f, i): h for f, i, h in rec["sites"]}
    for key, h in found.items():
        assert key in listed, f"unlisted site {key}"
        assert text_hash(listed[key]["text"]) == h, f"{key}: the reference line changed"
    assert set(found) == set(listed), sorted(set(listed) - set(found))


def _header_decls():
    hdr = open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(wl_\w+)\s*\(([^;{]*?)\)\s*;", hdr):
        args = m.group(2).strip()
        out[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",")])
    return out


def test_ccalls_name_declared_symbols_with_the_declared_arity():
    src = open(JL, encoding="utf-8").read()
    decl = _header_decls()
    calls = list(re.finditer(r"ccall\(\(:(\w+), libwlhip\), (\w+(?:\{\w+\})?), \(", src))
    assert len(calls) >= 60
    for m in calls:
        name = m.group(1)
        assert name in decl, f"{name} is not declared in include/wlhip.h"
        # argument-type tuple: balanced parentheses from the opening one
        i = m.end() - 1
        depth, k = 0, i
        while True:
            depth += src[k] == "("
            depth -= src[k] == ")"
            if depth == 0:
                break
            k += 1
        tup = src[i + 1:k]
        parts, d, cur = [], 0, ""
        for ch in tup:
            d += ch in "({"
            d -= ch in ")}"
            if ch == "," and d == 0:
                parts.append(cur); cur = ""
            else:
                cur += ch
        if cur.strip():
            parts.append(cur)
        assert len(parts) == decl[name], f"{name}: ccall passes {len(parts)} arguments, the header declares {decl[name]}"


def test_struct_mirrors_match_the_header():
    src = open(JL, encoding="utf-8").read()
    hdr = open(os.path.join(ROOT, "include", "wlhip.h"), encoding="utf-8").read()
    g = re.search(r"struct WlGrid; (.*?) end", src).group(1)
    assert [f.split("::")[0].strip() for f in g.split(";") if f.strip()] == ["D", "nx", "ny", "nz", "k0", "k1", "gk", "gnz"]
    d = re.search(r"struct WlSimDesc\n(.*?)\nend", src, re.S).group(1)
    fields = [f.split("::")[0].strip() for f in re.split(r"[;\n]", d) if "::" in f]
    assert fields == ["D", "dims", "uBC", "nu", "dt0", "perdir_mask", "exitBC", "scheme", "has_body", "u", "u0", "f", "p", "sigma", "V", "mu0", "mu1", "us"]
    body = re.search(r"typedef struct wl_sim_desc \{(.*?)\} wl_sim_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    cf = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        names = stmt.split(None, 1)[1]
        cf += [re.sub(r"[\*\s]|\[\d+\]", "", n) for n in names.split(",")]
    assert cf == fields
    b = re.search(r"struct WlBody; (.*?) end", src).group(1)
    assert [f.split("::")[0].strip() for f in b.split(";") if f.strip()] == ["kind", "c", "R", "m", "V"]


def test_dispatch_hazards_desk_check():
    src = open(JL, encoding="utf-8").read()
    code = "\n".join(l.split("#")[0] for l in src.split("\n"))          # comments stripped
    # (a) BroadcastStyle: Base owns  BroadcastStyle(a::AbstractArrayStyle{Any}, ::DefaultArrayStyle) = a ; a binding method whose second slot is
    #     ::AbstractArrayStyle (or untyped) would be ambiguous with it for every `hiparray .op scalar`.  Allowed: the one-argument Type form and
    #     methods whose second slot is exactly ::DefaultArrayStyle (strictly more specific than Base's).
    meths = re.findall(r"BroadcastStyle\(([^)]*)\)\s*=", code)
    assert meths, "the binding defines its broadcast style"
    for sig in meths:
        args = [a.strip() for a in sig.split(",")]
        if len(args) == 1:
            assert args[0].startswith("::Type{<:HipArray}"), sig
        else:
            assert len(args) == 2 and args[0] == "::HipStyle" and args[1] == "::Base.Broadcast.DefaultArrayStyle", f"ambiguous with Base: BroadcastStyle({sig})"
    # (b) no dictionary keyed by device arrays: AbstractArray keys hash through scalar getindex (one wl_d2h per element)
    assert not re.search(r"(WeakKeyDict|IdDict|Dict)\s*\{\s*(Any|HipArray|HA)", code)
    assert re.search(r"has_body\(a::HFlow\) = a\.μ₁\.bodied", code) and code.count("a.μ₁.bodied = true") == 2
    # (c) the composite step does not index device arrays element-wise
    step = re.search(r"function mom_step!\(a::HFlow\{D\}, b::HipMultiLevel.*?\nend\n", code, re.S).group(0)
    comp = re.search(r"function composite!\(a::HFlow\{D\}, b::HipMultiLevel.*?\nend\n", code, re.S).group(0)
    for body in (step, comp):
        assert not re.search(r"\ba\.(u|u⁰|p|σ|f|V|μ₀|μ₁)\[", body)
    # (d) every flow hands its spare velocity array to the library (exitBC flows included): `u⁰ .= u` stays a pointer rotation
    assert "a.μ₁.ptr, spare.ptr))" in comp and "Ptr{Cfloat}(C_NULL) : spare.ptr" not in comp
    assert 'b.spare.ptr = simfield(sim, "us")' in step and "!a.exitBC" not in step
    # (e) closures that are uniform in x keep the composite path: tabulated per step through wl_sim_set_forcing
    assert "(:wl_sim_set_forcing, libwlhip)" in code and "uniform_in_x(a.uBC" in step and "set_forcing!(sim, a)" in step
