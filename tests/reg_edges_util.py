"""Shared by the register-edge tests: the generated schedule header as Python lists."""
import re


def parse_header(text):
    """{code: {array or constant name: list or int}}"""
    out = {}
    for m in re.finditer(r"struct (\w+) \{\n(.*?)\n\};", text, re.S):
        d = {}
        for a in re.finditer(r"static constexpr int (\w+)\[\d+\] = \{([^}]*)\};", m.group(2)):
            d[a.group(1)] = [int(x) for x in a.group(2).split(",")]
        for a in re.finditer(r"(\w+) = (-?\d+)[,;]", m.group(2)):
            d[a.group(1)] = int(a.group(2))
        out[m.group(1)] = d
    return out
