#!/usr/bin/env python3
"""Whether two device listings hold the same kernels with the same code: for a change that must leave the kernels alone.

  isa_same.py OLD.s NEW.s
reads two listings of one source file from `make asm` (multicore_hw2_amd/csrc) and compares them kernel by kernel.  Equal means:
the same set of kernel symbols, and for every kernel the same text from its entry label to the end of its
.amdhsa_kernel ... .end_amdhsa_kernel block (the code, then registers, LDS, scratch and kernel-argument sizes).  The order of the
kernels in a file follows the order in which the host code names them, and the compiler numbers its labels by that order
(.LBB<function>_<block>, .Lfunc_end<function>), so the function number is taken out of every such label and of every mention of
one before the texts are compared.  The printer sets a block label's comment at a fixed column, so the blanks between the two
follow the label's length — one fewer where the function number gains a digit; that run of blanks is made one.  Nothing else is
taken out.  Text only: the tool knows no instruction.

Prints one verdict line, above it the names of kernels that differ or are in one listing only; exit status 1 on any difference."""
import re
import sys

_ENTRY = re.compile(r"^([A-Za-z_$][\w$.]*):")                       # a function's entry label (local labels start with .L)
_END = re.compile(r"^\.Lfunc_end\d+:")
_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_BLOCK = re.compile(r"(\.L|\b)BB\d+_(\d+)")                        # .LBB3_7 and, in comments, BB3_7
_FUNC = re.compile(r"\.Lfunc_(begin|end)\d+")
_PAD = re.compile(r"^(\.LBB_\d+:)[ \t]+;", re.M)                   # a block label (number taken out) and its comment


def kernels(text):
    """{kernel symbol: its text from the entry label to .end_amdhsa_kernel, labels in per-kernel form}."""
    out = {}
    name, lines, kernel = None, [], None
    for line in text.splitlines():
        m = _ENTRY.match(line)
        if m:   # (a data symbol's label too: nothing of it is kept, no .Lfunc_end follows it)
            name, lines, kernel = m.group(1), [line], None
            continue
        if name is None:
            continue
        if _END.match(line):
            if kernel is not None:
                if kernel != name or name in out:
                    raise ValueError("kernel %s: descriptor of %s, or listed twice" % (name, kernel))
                body = "\n".join(l.rstrip() for l in lines)
                out[name] = _PAD.sub(r"\1 ;", _FUNC.sub(r".Lfunc_\1", _BLOCK.sub(r"\1BB_\2", body)))
            name = None
            continue
        lines.append(line)
        m = _KERNEL.match(line)
        if m:
            kernel = m.group(1)
    return out


def compare(old_text, new_text):
    """(equal, kernels in both, [names that differ], [only in old], [only in new])"""
    a, b = kernels(old_text), kernels(new_text)
    differ = sorted(k for k in a if k in b and a[k] != b[k])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    return bool(a) and not (differ or only_a or only_b), len(set(a) & set(b)), differ, only_a, only_b


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    with open(argv[1]) as f:
        old = f.read()
    with open(argv[2]) as f:
        new = f.read()
    equal, both, differ, only_a, only_b = compare(old, new)
    for tag, names in (("differs", differ), ("only in " + argv[1], only_a), ("only in " + argv[2], only_b)):
        for k in names:
            print("%s: %s" % (tag, k))
    if equal:
        print("%s vs %s: EQUAL — %d kernels, the same symbols, code and descriptors" % (argv[1], argv[2], both))
        return 0
    print("%s vs %s: DIFFERENT — %d kernels differ, %d only in the first, %d only in the second (%d in both)"
          % (argv[1], argv[2], len(differ), len(only_a), len(only_b), both))
    return 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
