// yaml_lite.hpp — the subset of YAML the reference's scene files use (serde_yaml is not available). A text either
// means what YAML says it means or is refused with a line number; it is never read as something else
// (tests/test_yaml_differential.py holds that against PyYAML's composer).
//
// Read: block maps and block lists by indentation (a list may sit at its parent key's indentation), `- ` items that open a
// map or a list on the same line, one-line flow `[a, b]` / `{k: v}` collections, nested, with a trailing comma; plain
// scalars (a quote character inside one is an ordinary character), single-quoted scalars with `''`, double-quoted scalars
// with the escapes of YAML 1.2 (\x, \u, \U decoded to UTF-8); `#` comments (at the start of a line or behind a blank),
// blank lines, tabs as separation, CRLF, a UTF-8 byte order mark, one `---` and a closing `...`.
//
// Refused, each with its line: anchors, aliases, tags, block scalars (| >), complex keys (?), directives (%), a second
// document, content on the `---` line, scalars and flow collections that continue on the next line, `key: value` inside a
// flow sequence, a flow-map key without a value, a collection as a key, duplicate keys of one map (both lines named),
// `: ` inside a plain scalar, a plain scalar that starts with an indicator (`- `, `,`, `]`, `}`, `@`, backtick), an empty
// flow-sequence entry, an unknown escape, a tab as indentation, indentation that matches no open block.
#pragma once
#include <string>
#include <utility>
#include <vector>

namespace yaml_lite {

struct Node {
    enum Kind { Null, Scalar, Map, List } kind = Null;
    std::string scalar;
    bool quoted = false;
    std::vector<std::pair<std::string, Node>> map;
    std::vector<Node> list;
    int line = 0;
    const Node* find(const std::string& key) const {
        for (auto& kv : map)
            if (kv.first == key) return &kv.second;
        return nullptr;
    }
    bool is_null() const {
        return kind == Null || (kind == Scalar && !quoted && (scalar == "~" || scalar == "null" || scalar == "Null" ||
                                                              scalar == "NULL" || scalar.empty()));
    }
};

// Throws std::runtime_error with a line number on malformed input.
Node parse(const std::string& text);

}  // namespace yaml_lite
