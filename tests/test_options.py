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
                   ("line_zl512", 16), ("fused_minw", 2), ("no_such_option", 0), (None, 0)]
        for key, value in refused:
            assert _set(key, value) == OCN_EINVAL, (key, value)
        # the edges of the ranges are accepted
        for key, value in [("tendency_impl", 0), ("arithmetic", 1), ("epilogue_rows", 1), ("epilogue_rows", 8), ("line_zl512", 8)]:
            assert _set(key, value) == 0, (key, value)
    finally:
        for key, (_alias, default, _scope) in doc.items():
            assert _set(key, default) == 0, key
