"""Regenerate the appendix of INTEGRATION.md: one row per entry point of include/ocn_mi355x.h with the Julia `ccall` type tuple a binder
writes (python tools/gen_integration_table.py). The prose sections above the marker line are kept."""
import os
import re
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = "## 6. Every entry point and its `ccall` signature"
hdr = open(os.path.join(ROOT, "include", "ocn_mi355x.h")).read()
body = hdr[hdr.index("extern \"C\""):]
body = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)) if "\n" not in m.group(0) else "\n" * m.group(0).count("\n"), body, flags=re.S)
decls = re.findall(r"((?:const\s+)?(?:int|void|char|double)\s*\*?\s*)(ocn_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", body, flags=re.S)


def jl_type(t):
    t = " ".join(t.replace("const", " ").split())
    name = re.sub(r"\[\d*\]", "", t.split()[-1].lstrip("*")) if t else ""
    core = t
    if "(*" in core:                                   # const int (*locs)[3]
        return "Ptr{Cint}"
    ptr = core.count("*") + core.count("[")
    base = core.split()[0] if core else ""
    if base in ("ocn_grid_t", "ocn_poisson_t", "ocn_model_t", "ocn_dist_t", "ocn_dist_poisson_t"):
        return "Ptr{Ptr{Cvoid}}" if ptr else "Ptr{Cvoid}"
    if base == "ocn_bc_t":
        return "Ptr{OcnBC}"
    if base == "ocn_forcing_t":
        return "Ptr{OcnForcing}"
    if base == "ocn_transport_t":
        return "Ptr{OcnTransport}"
    if base == "ocn_operand_t":
        return "Ptr{OcnOperand}"
    if base == "ocn_expr_ins_t":
        return "Ptr{OcnExprIns}"
    if base == "ocn_stencil_ins_t":
        return "Ptr{OcnStencilIns}"
    if base == "ocn_stencil_operand_t":
        return "Ptr{OcnStencilOperand}"
    if base == "ocn_time_fold_t":
        return "Ptr{OcnTimeFold}"
    if base == "char":
        return "Ptr{Cstring}" if ptr > 1 else "Cstring"
    if base == "void":
        return "Ptr{Ptr{Cvoid}}" if ptr > 1 else "Ptr{Cvoid}"
    scalar = {"int": "Cint", "double": "Cdouble", "size_t": "Csize_t", "long": "Clong", "int64_t": "Int64", "unsigned": "Cuint", "uint8_t": "UInt8", "uint16_t": "UInt16"}.get(base, base)
    if ptr >= 2:
        return "Ptr{Ptr{%s}}" % scalar
    if ptr == 1:
        return "Ptr{%s}" % scalar
    return scalar


rows = []
for ret, name, args in decls:
    args = " ".join(args.split())
    types = [] if args in ("", "void") else [jl_type(a.strip()) for a in re.split(r",(?![^()]*\))", args)]
    r = " ".join(ret.split())
    rt = "Cstring" if "char" in r else ("Ptr{Cvoid}" if "void" in r and "*" in r else ("Cvoid" if r.startswith("void") else "Cint"))
    tup = "(" + ", ".join(types) + ("," if len(types) == 1 else "") + ")"
    rows.append(f"| `{name}` | `ccall((:{name}, libocn), {rt}, {tup}, …)` |")
table = [MARK, "",
         "Generated from `include/ocn_mi355x.h` by `tools/gen_integration_table.py` (%d entry points; the header's comment on each one cites the" % len(rows),
         "reference function it replaces). Handles are `Ptr{Cvoid}`, device arrays are passed as `Ptr{Cdouble}` obtained from",
         "`pointer(parent(field.data))`, arrays of device pointers as `Ptr{Ptr{Cdouble}}` built on the host; `OcnBC` / `OcnTransport` mirror",
         "`ocn_bc_t` / `ocn_transport_t` field by field (`struct OcnBC; kind::Cint; value::Cdouble; array::Ptr{Cdouble}; end`). Every `Cint`",
         "return is a status: `check(rc)` of §1. `OcnForcing` mirrors `ocn_forcing_t` the same way; its mask and target tables are host",
         "`Vector{Float64}`s the binder fills with the reference's own `GaussianMask` / `PiecewiseLinearMask` / `LinearTarget` at the field's nodes.",
         "`OcnOperand` mirrors `ocn_operand_t` (`op::Cint; a::Ptr{Cdouble}; b::Ptr{Cdouble}; ca::Cdouble; cb::Cdouble; loc_a, loc_b, loc::NTuple{3, Cint}`),",
         "filled from a `BinaryOperation`'s `op`, `a`, `b` and the locations of the three. `OcnExprIns` mirrors `ocn_expr_ins_t`",
         "(`op::Cint; a::Cint; b::Cint; c::Cint; imm::Cdouble`): one recorded operation of a boundary function. `OcnStencilIns` mirrors",
         "`ocn_stencil_ins_t` (`op, a, b, c, di, dj, dk::Cint; imm::Cdouble`): one recorded operation of a kernel function, and",
         "`OcnStencilOperand` mirrors `ocn_stencil_operand_t` (`program::Ptr{OcnStencilIns}; n::Cint; args::Ptr{Ptr{Cdouble}};",
         "arg_locs::Ptr{Cint}; nargs::Cint; loc::NTuple{3, Cint}`), filled from a `KernelFunctionOperation`'s recorded program and arguments.",
         "`OcnTimeFold` mirrors `ocn_time_fold_t` (`T_previous::Cdouble; dt::Cdouble; T_current::Cdouble; first::Cint`): the three times of",
         "`accumulate_result!` and whether the sample is the first of its window.", "", "| entry point | binding |", "|---|---|"] + rows
p = os.path.join(ROOT, "INTEGRATION.md")
s = open(p).read()
if MARK in s:
    s = s[:s.index(MARK)].rstrip() + "\n\n"
else:
    s = s.rstrip() + "\n\n"
open(p, "w").write(s + "\n".join(table) + "\n")
print(len(rows), "entry points")
