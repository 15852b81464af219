"""CPU-only text check on starst3r_amd/csrc: a function with external linkage that one .hip file defines and another
calls is declared in a header (stages.h, radix_sort.h, common.h), never by a prototype copied into a .hip file -- a copy
that drifts from the definition is noticed by nobody but the linker, and only if the mangled names differ."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "starst3r_amd", "csrc")
# a statement that starts a line (indented or not, `extern "C"` in front or not) with a return type followed by
# st3r_<name>( -- `return st3r_x(...);` and `rc = st3r_x(...);` are calls, `static` ones are file-local
HEAD = re.compile(r"^[ \t]*(?:extern\s+\"C\"\s+)?(?!static\b|return\b|else\b)[A-Za-z_][\w:<>*&]*[\w:<>*&\s]*?[\s*&]st3r_\w+\(",
                  re.M)


def _bodyless_declarations(text):
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    found = []
    for m in HEAD.finditer(text):
        end = re.compile(r"[;{]").search(text, m.end())
        # `);` before any `{`: a declaration.  (A definition reaches its `{` first; so does an exported one.)
        if end and end.group(0) == ";" and text[:end.start()].rstrip().endswith(")"):
            found.append((text.count("\n", 0, m.start()) + 1, " ".join(text[m.start():end.start() + 1].split())[:100]))
    return found


def test_the_check_sees_a_copied_prototype():
    sample = ("int st3r_a_impl(int x) {\n    return st3r_b(x);\n}\n"
              "int st3r_b_impl(hipStream_t s, int N,\n                const float* means);   // other.hip\n"
              "static int st3r_c_impl(int x);\n"
              "ST3R_EXPORT int st3r_d(int x) {\n    int rc = st3r_a_impl(x);\n    return rc;\n}\n"
              "extern \"C\" int st3r_e(int x);\n"
              "namespace n {\n    const char* st3r_f(void);\n}\n")
    assert [line for line, _ in _bodyless_declarations(sample)] == [4, 11, 13]


def test_no_hip_file_declares_another_files_function():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")))
    assert len(files) >= 20, files
    bad = {os.path.basename(f): d for f in files if (d := _bodyless_declarations(open(f).read()))}
    assert not bad, f"prototypes of external-linkage st3r_* functions in .hip files (declare them in stages.h): {bad}"
