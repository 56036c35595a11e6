"""csrc/sketch.hip holds the ring kernel twice: sketch_ring_kernel (columns a
range; C5 rides on it, so it stays as it compiles) and sketch_ring_cols_kernel
(columns an index list), a copy with the places that name a column changed. A
fix to the ring has to reach both. This test strips the comments of the two
bodies and requires that they differ in those places only: the tile index, the
tile's early exit, the metadata fill, the pair's validity and the output slot."""
import difflib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what the range kernel says there -> what the column-list kernel says
ONLY_IN_RANGE = [
    "int tr, tcb;",
    "if (tri) {",
    "int64_t a = (int64_t)((__builtin_sqrt(8.0 * (double)bt + 1.0) - 1.0) * 0.5);",
    "while (a * (a + 1) / 2 > bt) a--;",
    "while ((a + 1) * (a + 2) / 2 <= bt) a++;",
    "tcb = (int)a;",
    "tr = (int)(bt - a * (a + 1) / 2);",
    "} else {",
    "tr = (int)(bt / tiles_c);",
    "tcb = (int)(bt % tiles_c);",
    "}",
    "const int64_t row0 = r0 + (int64_t)tr * R, col0 = c0 + (int64_t)tcb * C;",
    "if (upper && col0 + C - 1 <= row0) return;",
    "const int64_t gi = s < R ? row0 + s : col0 + (s - R);",
    "const bool ok = s < R ? gi < r1 : gi < c1;",
    "const bool valid = i < r1 && j < c1 && !(upper && j <= i);",
    "const int64_t o = (i - r0) * ld + (j - c0);",
]
ONLY_IN_COLS = [
    "const int tr = (int)(bt / tiles_c), tcb = (int)(bt % tiles_c);",
    "const int64_t row0 = r0 + (int64_t)tr * R, col0 = (int64_t)tcb * C;",
    "const int64_t p = s < R ? row0 + s : col0 + (s - R);",
    "const bool ok = s < R ? p < r1 : p < ncols;",
    "const int64_t gi = s < R || !ok ? p : cols[p];",
    "const bool valid = i < r1 && j < ncols;",
    "const int64_t o = (i - r0) * ld + j;",
]


def body_of(text, name):
    """The lines of kernel `name` from the line after its `{` to its closing
    `}` at column 0, comments and blank lines dropped, whitespace folded."""
    start = text.index("void %s(" % name)
    start = text.index(") {\n", start) + 4
    end = text.index("\n}\n", start)
    out = []
    for line in text[start:end].split("\n"):
        line = " ".join(re.sub(r"//.*", "", line).split())
        if line:
            out.append(line)
    return out


def test_ring_kernels_differ_only_where_they_name_a_column():
    with open(os.path.join(ROOT, "genome.distance_amd", "csrc", "sketch.hip")) as f:
        text = f.read()
    a, b = body_of(text, "sketch_ring_kernel"), body_of(text, "sketch_ring_cols_kernel")
    assert len(a) > 150 and len(b) > 150
    gone, new = [], []
    for line in difflib.ndiff(a, b):
        if line.startswith("- "):
            gone.append(line[2:])
        elif line.startswith("+ "):
            new.append(line[2:])
    assert gone == ONLY_IN_RANGE, gone
    assert new == ONLY_IN_COLS, new
