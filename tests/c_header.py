"""What the header tests share: include/spmvHip.h without its comments, its struct typedefs and prototypes, and a C program
compiled against it and run (gcc only, no GPU)."""
import os
import re
import subprocess

from conftest import ROOT

INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "spmvHip.h")


def code(path=HEADER):
    """the file's text without /* */ comments"""
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def structs(path=HEADER):
    """{typedef name: [field names in order]} of every `typedef struct { ... } NAME;`"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*(\w+)\s*;", code(path), re.S):
        out[name] = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:\[\w+\])?\s*(?:,|$)", decl.strip())]
    return out


def prototypes(path=HEADER):
    """{function name: number of parameters} of every prototype, those declared through a function typedef
    (`typedef int (SPMV_HIP)(...);  SPMV_HIP name;`) included"""
    text = re.sub(r"typedef\s+struct\s*\{[^}]*\}\s*\w+\s*;", "", code(path), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)

    def count(params):
        return 0 if params.strip() in ("", "void") else params.count(",") + 1
    kinds = {name: count(params) for name, params in re.findall(r"typedef\s+\w+\s*\(\s*(\w+)\s*\)\s*\(([^()]*)\)\s*;", text)}
    text = re.sub(r"^\s*typedef\b[^;]*;", "", text, flags=re.M)
    out = {name: count(params) for name, params in re.findall(r"\b(\w+)\s*\(([^()]*)\)\s*;", text)}
    for kind, name in re.findall(r"^\s*(\w+)\s+(\w+)\s*;", text, re.M):
        if kind in kinds:
            out[name] = kinds[kind]
    return out


def run_c(tmp_path, body, name="probe"):
    """compile `int main(void) { body }` against include/spmvHip.h, run it, return what it printed"""
    src, exe = tmp_path / (name + ".c"), tmp_path / name
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spmvHip.h"\nint main(void) {\n' + body + "    return 0;\n}\n")
    subprocess.run(["gcc", "-I" + INCLUDE, "-o", str(exe), str(src)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
