#!/usr/bin/env python3
"""Writes tests/golden/yaml_corpus.json: the YAML texts of tests/yaml_cases.py and the trees PyYAML's composer builds from
them (or the fact that it raises). tests/test_yaml_differential.py reads the fixture, so that the test itself needs no PyYAML.

    python tests/golden/make_yaml_corpus.py

The generator defines the classes, so they are checked here before anything is written: PyYAML accepts every `in` and every
`outside` text, and refuses every entry of the hand-curated malformed table.
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import yaml_cases  # noqa: E402

OUT = HERE / "yaml_corpus.json"


def dumps(corpus) -> str:
    return json.dumps(corpus, ensure_ascii=True, separators=(",", ":"), sort_keys=True).replace('},{"cls"', '},\n{"cls"') + "\n"


def main():
    corpus = yaml_cases.corpus()
    for c in corpus["cases"]:
        if c["cls"] in ("in", "outside"):
            assert "tree" in c["expect"], f"PyYAML refuses {c['id']}: {c['text']!r}"
        if c["cls"] == "bad-table":
            assert "error" in c["expect"], f"PyYAML accepts {c['id']}: {c['text']!r} -> {c['expect']}"
    text = dumps(corpus)
    OUT.write_text(text)
    n = {k: sum(c["cls"] == k for c in corpus["cases"]) for k in ("in", "outside", "bad-table", "bad-mutation")}
    print(f"{OUT.name}: {len(text)} bytes, {n}")


if __name__ == "__main__":
    main()
