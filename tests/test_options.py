"""CPU: the tuning options (include/ocn_mi355x.h: ocn_set_option) are one table (csrc/ocn_api.hip: kOptions) over one struct
(csrc/ocn_options.h). The header's list of keys is that table -- names, aliases, scopes and defaults -- and the library accepts every key
at its documented default and refuses what the table refuses. ocn_set_option works before ocn_init: no GPU is needed."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "oldoceananigans.jl_amd", "csrc")
OCN_EINVAL = -1


def _documented():
    """{key: (alias, default, scope)} from the header's list"""
    text = open(os.path.join(ROOT, "include", "ocn_mi355x.h")).read()
    rows = re.findall(r'^ \*   "(\w+)"(?: \(alias "(\w+)"\))? = (-?\d+) \((step|creation|partitioned)\):', text, flags=re.M)
    return {k: (alias or None, int(d), scope) for k, alias, d, scope in rows}


def _table():
    """{key: (alias, member default, scope)} from kOptions and the member initialisers of OcnOptions"""
    src = open(os.path.join(CSRC, "ocn_api.hip")).read()
    block = src[src.index("static const OptionRow kOptions[] = {"):]
    block = block[:block.index("\n};")]
    defaults = {m: int(v) for m, v in re.findall(r"^\s+int (\w+) = (-?\d+);", open(os.path.join(CSRC, "ocn_options.h")).read(), flags=re.M)}
    out = {}
    for line in block.splitlines()[1:]:
        key, member, scope = re.match(r'\s+\{"(\w+)", &OcnOptions::(\w+), OPT_(\w+)', line).groups()
        alias = re.search(r', "(\w+)"\},$', line)
        out[key] = (alias.group(1) if alias else None, defaults[member], scope.lower())
    return out


def _set(key, value):
    from oldoceananigans_jl_amd import _lib
    return _lib.lib().ocn_set_option(None if key is None else key.encode(), int(value))


def test_the_header_documents_exactly_the_table():
    doc, table = _documented(), _table()
    assert len(table) >= 30
    assert doc == table


def test_every_key_is_accepted_at_its_default_and_bad_values_are_refused():
    doc = _documented()
    try:
        for key, (alias, default, _scope) in doc.items():
            assert _set(key, default) == 0, key
            if alias:
                assert _set(alias, default) == 0, alias
        refused = [("tendency_impl", -1), ("tendency_impl", 3), ("arithmetic", -1), ("arithmetic", 2), ("role_kchunk", -1),
                   ("fused_kchunk", -1), ("epilogue_kchunk", -1), ("epilogue_rows", 0), ("epilogue_rows", 9), ("line_zl512", 5),
                   ("line_zl512", 16), ("fused_minw", 2), ("no_such_option", 0), (None, 0),
                   ("fused_ty", 5), ("fused_ty", 0), ("fused_ty", 8), ("role_ldspad", -1), ("role_ldspad", 148257), ("role_ldspad", 1 << 30),
                   ("async_halos", -2), ("async_halos", 2), ("strip_width", -1)]
        # every switch is 0 or 1: a key whose documented text gives no range
        switches = [k for k in doc if k not in ("tendency_impl", "arithmetic", "role_kchunk", "role_ldspad", "fused_ty", "fused_kchunk", "epilogue_rows",
                                                "epilogue_kchunk", "line_zl512", "async_halos", "strip_width")]
        assert len(switches) == 27
        refused += [(k, v) for k in switches for v in (-1, 2)] + [("dist_fused_step", 2)]
        for key, value in refused:
            assert _set(key, value) == OCN_EINVAL, (key, value)
        # the edges of the ranges are accepted
        edges = [("tendency_impl", 0), ("arithmetic", 1), ("epilogue_rows", 1), ("epilogue_rows", 8), ("line_zl512", 8), ("fused_ty", 3),
                 ("role_ldspad", 148256), ("async_halos", -1), ("async_halos", 0), ("async_halos", 1), ("strip_width", 64)]
        for key, value in edges + [(k, v) for k in switches for v in (0, 1)]:
            assert _set(key, value) == 0, (key, value)
    finally:
        for key, (_alias, default, _scope) in doc.items():
            assert _set(key, default) == 0, key


def test_every_key_has_a_variant_test():
    """tests/option_variants.py has one row per key of kOptions -- a new option without a row fails here --; a row that names an existing
    test names one that exists; every value the GPU tests run is one the library accepts, and the row's default is the member's"""
    import option_variants as V
    table = _table()
    assert set(V.VARIANTS) == set(table), set(V.VARIANTS) ^ set(table)
    tests = os.path.join(ROOT, "tests")
    try:
        for key, row in V.VARIANTS.items():
            assert len(row) == 1 or set(row) == {"default", "values"}, key
            if "test" in row:
                fname, name = row["test"].split("::")
                assert re.search(r"^def %s\(" % re.escape(name), open(os.path.join(tests, fname)).read(), flags=re.M), row["test"]
                assert '"%s"' % key in open(os.path.join(tests, fname)).read(), (key, fname)
            elif "reason" in row:
                assert row["reason"].strip(), key
            else:
                assert row["default"] == table[key][1], key
                assert row["values"] and row["default"] not in row["values"], key
                for value in row["values"]:
                    assert _set(key, value) == 0, (key, value)
    finally:
        for key, (_alias, default, _scope) in table.items():
            assert _set(key, default) == 0, key
