"""Rewrite GLSL compute-shader text into text a C++20 compiler accepts after
oracle/glsl_prelude.hpp — TEST INFRASTRUCTURE ONLY.

    python3 oracle/glsl_rewrite.py IN.glsl OUT.inc

Token rules only; nothing here knows what the shader computes:
  * comments are dropped (a URL in one must not look like a swizzle);
  * the `#version` line is dropped;
  * a decimal floating literal without a suffix gets `f` (GLSL's are float);
  * a swizzle `.xyz` / `.rgb` / `.stp` (2-4 letters of one set) becomes the
    call `.xyz()` that GLM's swizzle members answer to;
  * the scalar constructor `int(` becomes the prelude's `glsl_int(`: a C++ cast
    of a float outside the int range is undefined behaviour, and the shader
    performs such casts (their results unused) in every floor shadow.
The output goes under oracle/_ref/ (git-ignored): it is the reference's program
text and is never committed.
"""
import re
import sys

_TOKEN = re.compile(r"""
    (?P<comment>//[^\n]*|/\*.*?\*/)
  | (?P<version>^[ \t]*\#[ \t]*version[^\n]*$)
  | (?P<float>(?<![\w.])(?:\d+\.\d*|\.\d+)(?:[eE][+-]?\d+)?(?![\w.])
             |(?<![\w.])\d+[eE][+-]?\d+(?![\w.]))
  | (?P<swizzle>\.(?:[xyzw]{2,4}|[rgba]{2,4}|[stpq]{2,4})\b(?!\s*\())
  | (?P<intctor>(?<![\w.])int(?=\s*\())
""", re.X | re.S | re.M)


def _sub(m: "re.Match[str]") -> str:
    kind = m.lastgroup
    text = m.group(0)
    if kind == "comment":
        return " " if "\n" not in text else "\n" * text.count("\n")
    if kind == "version":
        return ""
    if kind == "float":
        return text + "f"
    if kind == "swizzle":
        return text + "()"
    return "glsl_int"


def rewrite(src: str) -> str:
    return _TOKEN.sub(_sub, src)


def main(argv) -> int:
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    with open(argv[1], encoding="utf-8") as fh:
        src = fh.read()
    with open(argv[2], "w", encoding="utf-8") as fh:
        fh.write(rewrite(src))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
