"""Statement lines of Python files: the lines that hold a token of code, i.e. that are neither blank, nor a comment, nor part of a docstring
(the docstrings found by an ast walk).  The size measure of DESIGN 29.

    python scripts/statement_lines.py phosphorus_mk2_amd/xpu.py phosphorus_mk2_amd/device.py phosphorus_mk2_amd/film.py"""
import ast
import io
import sys
import tokenize

NOT_CODE = {tokenize.COMMENT, tokenize.NL, tokenize.NEWLINE, tokenize.INDENT, tokenize.DEDENT, tokenize.ENCODING, tokenize.ENDMARKER}


def statement_lines(source):
    docstrings, code = set(), set()
    for node in ast.walk(ast.parse(source)):
        if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and ast.get_docstring(node, clean=False) is not None:
            docstrings.update(range(node.body[0].lineno, node.body[0].end_lineno + 1))
    for tok in tokenize.generate_tokens(io.StringIO(source).readline):
        if tok.type not in NOT_CODE:
            code.update(range(tok.start[0], tok.end[0] + 1))
    return len(code - docstrings)


if __name__ == "__main__":
    counts = [(path, statement_lines(open(path).read())) for path in sys.argv[1:]]
    for path, n in counts:
        print(f"{n:6d} {path}")
    print(f"{sum(n for _, n in counts):6d} total")
