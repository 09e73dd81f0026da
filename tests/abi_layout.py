"""A public header's structs against their ctypes mirrors: sizeof and every offsetof, as a C compiler sees them."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def c_layout(tmp_path, headers, structs, extra=""):
    """{"Name": sizeof, "Name.field": offsetof, ...} as strings, printed by a C program that includes ``headers``;
    ``structs``: C name -> ctypes mirror (its field names are the C ones).  ``extra``: further C statements, whose
    "key value" lines are in the result too."""
    lines = []
    for cname, t in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in t._fields_]
    src = tmp_path / "p.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n" + "".join(f'#include "{h}"\n' for h in headers)
                   + "int main(void){" + "".join(lines) + extra + " return 0;}\n")
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "p")], check=True)
    out = subprocess.run([str(tmp_path / "p")], capture_output=True, text=True, check=True).stdout
    return dict(l.rsplit(" ", 1) for l in out.splitlines())


def ctypes_layout(structs):
    want = {}
    for cname, t in structs.items():
        want[cname] = str(C.sizeof(t))
        want.update({f"{cname}.{f}": str(getattr(t, f).offset) for f, _ in t._fields_})
    return want
