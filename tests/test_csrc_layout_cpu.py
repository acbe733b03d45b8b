"""The layout rule of libcontinual_amd/csrc, as text (no compiler, no library, no device): a host function that one .hip file defines for another is declared
once, in csrc/kernels.h, and nowhere else.  build.sh compiles with -Werror=missing-prototypes, which a stale hand-written prototype in a .hip file would satisfy
just as well as the header does -- so the prototypes themselves are looked for here."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libcontinual_amd", "csrc")
# a return type and `clhip_name(` at column 0 (behind `extern "C"` or not)
_HEAD = re.compile(r'^(?:extern "C" )?(?:[A-Za-z_][\w:<>]*[ \t*&]+)+(clhip_\w+)\(', re.M)


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _declarations(text):
    """(name, line, is_prototype) of every file-scope `type clhip_name(...)`: from the opening parenthesis to its match, then the next token -- `;` ends a
    prototype, `{` opens a definition"""
    out = []
    for m in _HEAD.finditer(text):
        i, depth = m.end(), 1
        while depth:
            depth += (text[i] == "(") - (text[i] == ")")
            i += 1
        while text[i].isspace():
            i += 1
        assert text[i] in ";{", (m.group(1), text[i])
        out.append((m.group(1), text.count("\n", 0, m.start()) + 1, text[i] == ";"))
    return out


def _hip_files():
    names = sorted(n for n in os.listdir(CSRC) if n.endswith(".hip"))
    assert len(names) >= 31
    return names


def test_no_hip_file_declares_a_clhip_function_by_hand():
    found = [(n, line, name) for n in _hip_files() for name, line, proto in _declarations(_read(n)) if proto]
    assert found == []


def test_every_name_of_the_header_is_defined_in_exactly_one_hip_file():
    declared = _declarations(_read("kernels.h"))
    assert len(declared) >= 100 and all(proto for _, _, proto in declared)
    names = [name for name, _, _ in declared]
    assert len(names) == len(set(names))                              # ... and declared once
    defined = {}
    for n in _hip_files():
        for name, _, proto in _declarations(_read(n)):
            if not proto:
                defined.setdefault(name, []).append(n)
    assert {name: defined.get(name, []) for name in names if len(defined.get(name, [])) != 1} == {}


def test_build_script_watches_the_header_and_carries_the_flag():
    sh = _read("build.sh")
    rule = [l for l in sh.splitlines() if "-nt $OBJ/$f.o" in l]
    assert len(rule) == 1 and all(f"[ {h} -nt $OBJ/$f.o ]" in rule[0] for h in ("common.h", "kernels.h", "xch.h", "rp_tile.h"))
    flags = [l for l in sh.splitlines() if l.startswith("FLAGS=")]
    assert len(flags) == 1 and "-Werror=missing-prototypes" in flags[0].split()
