#include "yaml_lite.hpp"

#include <cstdint>
#include <stdexcept>

namespace yaml_lite {
namespace {

struct Line {
    int indent;
    std::string text;  // without indentation and trailing blanks; a trailing comment is still there
    int no;
};

[[noreturn]] void bad(int line, const std::string& what) {
    throw std::runtime_error("yaml: line " + std::to_string(line) + ": " + what);
}

bool blank(char c) { return c == ' ' || c == '\t'; }

std::string rstrip(std::string s) {
    while (!s.empty() && (blank(s.back()) || s.back() == '\r')) s.pop_back();
    return s;
}
std::string strip(const std::string& s) {
    size_t b = 0;
    while (b < s.size() && blank(s[b])) ++b;
    return rstrip(s.substr(b));
}

// A comment starts at a '#' that opens the text or follows a blank. Comments are recognised only where a scalar cannot
// continue (the scanners below call this), never by a pass over the raw line: a quote character inside a plain scalar
// (`it's # c`) is an ordinary character.
bool comment_at(const std::string& s, size_t i) { return i < s.size() && s[i] == '#' && (i == 0 || blank(s[i - 1])); }

bool is_dash_item(const std::string& t) { return t[0] == '-' && (t.size() == 1 || t[1] == ' '); }

std::vector<Line> split_lines(const std::string& text) {
    std::vector<Line> out;
    size_t pos = 0;
    int no = 0;
    int doc_line = 0, end_line = 0;  // the lines of the `---` and `...` markers met so far
    while (pos <= text.size()) {
        size_t e = text.find('\n', pos);
        if (e == std::string::npos) e = text.size();
        std::string s = rstrip(text.substr(pos, e - pos));
        pos = e + 1;
        ++no;
        size_t ind = 0;
        while (ind < s.size() && s[ind] == ' ') ++ind;
        if (ind < s.size() && s[ind] == '\t') {
            size_t k = ind;
            while (k < s.size() && blank(s[k])) ++k;
            if (k == s.size() || s[k] == '#') continue;  // blanks and a comment only
            bad(no, "tab used for indentation");
        }
        std::string body = s.substr(ind);
        if (body.empty() || body[0] == '#') continue;
        if (ind == 0 && body.compare(0, 3, "---") == 0 && (body.size() == 3 || blank(body[3]))) {
            size_t k = 3;
            while (k < body.size() && blank(body[k])) ++k;
            if (k < body.size() && !comment_at(body, k)) bad(no, "content on the line of a `---` marker is not supported");
            if (doc_line || !out.empty())
                bad(no, "a second document is not supported (the first began at line " +
                            std::to_string(doc_line ? doc_line : out.front().no) + ")");
            doc_line = no;
            continue;
        }
        if (ind == 0 && body.compare(0, 3, "...") == 0 && (body.size() == 3 || blank(body[3]))) {
            size_t k = 3;
            while (k < body.size() && blank(body[k])) ++k;
            if (k < body.size() && !comment_at(body, k)) bad(no, "content on the line of a `...` marker is not supported");
            if (!end_line) end_line = no;
            continue;
        }
        if (end_line) bad(no, "content after the document end marker `...` of line " + std::to_string(end_line) + " is not supported");
        if (ind == 0 && body[0] == '%') bad(no, "directives (%) are not supported");
        out.push_back(Line{int(ind), body, no});
    }
    return out;
}

void put_utf8(std::string& out, uint32_t cp) {
    if (cp < 0x80) {
        out += char(cp);
    } else if (cp < 0x800) {
        out += char(0xC0 | (cp >> 6));
        out += char(0x80 | (cp & 0x3F));
    } else if (cp < 0x10000) {
        out += char(0xE0 | (cp >> 12));
        out += char(0x80 | ((cp >> 6) & 0x3F));
        out += char(0x80 | (cp & 0x3F));
    } else {
        out += char(0xF0 | (cp >> 18));
        out += char(0x80 | ((cp >> 12) & 0x3F));
        out += char(0x80 | ((cp >> 6) & 0x3F));
        out += char(0x80 | (cp & 0x3F));
    }
}

// s[i] is the opening quote; returns the content and leaves i behind the closing quote. `''` inside single quotes is one
// apostrophe; inside double quotes the escapes of YAML 1.2 section 5.7 are decoded (\x, \u and \U to UTF-8) and any other
// escape is refused. A quoted scalar ends on its line.
std::string scan_quoted(const std::string& s, size_t& i, int line) {
    const char q = s[i++];
    std::string out;
    for (;;) {
        if (i >= s.size()) bad(line, "unterminated quoted string (a quoted scalar that continues on the next line is not supported)");
        const char c = s[i];
        if (c == q) {
            if (q == '\'' && i + 1 < s.size() && s[i + 1] == '\'') {
                out += '\'';
                i += 2;
                continue;
            }
            ++i;
            return out;
        }
        if (q == '"' && c == '\\') {
            if (i + 1 >= s.size()) bad(line, "unterminated quoted string (a line folded with `\\` is not supported)");
            const char e = s[i + 1];
            i += 2;
            int hex = 0;
            switch (e) {
                case '0': out += '\0'; break;
                case 'a': out += '\a'; break;
                case 'b': out += '\b'; break;
                case 't': case '\t': out += '\t'; break;
                case 'n': out += '\n'; break;
                case 'v': out += '\v'; break;
                case 'f': out += '\f'; break;
                case 'r': out += '\r'; break;
                case 'e': out += '\x1b'; break;
                case ' ': out += ' '; break;
                case '"': out += '"'; break;
                case '/': out += '/'; break;
                case '\\': out += '\\'; break;
                case 'N': put_utf8(out, 0x85); break;
                case '_': put_utf8(out, 0xA0); break;
                case 'L': put_utf8(out, 0x2028); break;
                case 'P': put_utf8(out, 0x2029); break;
                case 'x': hex = 2; break;
                case 'u': hex = 4; break;
                case 'U': hex = 8; break;
                default: bad(line, std::string("unknown escape `\\") + e + "` in a double-quoted string");
            }
            if (hex) {
                uint32_t cp = 0;
                for (int k = 0; k < hex; ++k, ++i) {
                    const char h = i < s.size() ? s[i] : 'x';
                    const int d = h >= '0' && h <= '9' ? h - '0' : h >= 'a' && h <= 'f' ? h - 'a' + 10 : h >= 'A' && h <= 'F' ? h - 'A' + 10 : -1;
                    if (d < 0) bad(line, std::string("`\\") + e + "` needs " + std::to_string(hex) + " hexadecimal digits");
                    cp = cp * 16 + uint32_t(d);
                }
                if (cp > 0x10FFFF || (cp >= 0xD800 && cp <= 0xDFFF)) bad(line, "escape names no Unicode scalar value");
                put_utf8(out, cp);
            }
            continue;
        }
        out += c;
        ++i;
    }
}

// What a plain scalar must not begin with: the indicators of YAML constructs outside the subset, by name.
void check_plain_start(const std::string& s, size_t i, int line) {
    const char c = s[i];
    const bool alone = i + 1 >= s.size() || blank(s[i + 1]);
    switch (c) {
        case '&': bad(line, "anchors (&) are not supported");
        case '*': bad(line, "aliases (*) are not supported");
        case '!': bad(line, "tags (!) are not supported");
        case '|': bad(line, "block scalars (|) are not supported");
        case '>': bad(line, "block scalars (>) are not supported");
        case '?': bad(line, "complex keys (?) are not supported");
        case '%': bad(line, "a plain scalar cannot start with `%` (directives are not supported)");
        case '@': case '`': bad(line, std::string("a plain scalar cannot start with the reserved character `") + c + "`");
        case ',': case ']': case '}': case '[': case '{':
            bad(line, std::string("unexpected `") + c + "`");
        case '-':
            if (alone) bad(line, "a block sequence entry (`- `) cannot start here");
            break;
        case ':':
            if (alone) bad(line, "a mapping value (`: `) without a key is not supported");
            break;
        default: break;
    }
}

bool flow_indicator(char c) { return c == ',' || c == '[' || c == ']' || c == '{' || c == '}'; }

// ---- flow / scalar parsing --------------------------------------------------------------------
struct Flow {
    const std::string& s;
    size_t i;
    int line;
    // blanks, and a comment up to the end of the line
    void ws() {
        while (i < s.size() && blank(s[i])) ++i;
        if (comment_at(s, i)) i = s.size();
    }
    void need_more(const char* what) {
        if (i >= s.size()) bad(line, std::string(what) + " (a flow collection that continues on the next line is not supported)");
    }
    // a ':' that ends a flow-map key or would open a single-pair map: followed by a blank, a flow indicator or the end
    bool value_colon(size_t k) const { return s[k] == ':' && (k + 1 >= s.size() || blank(s[k + 1]) || flow_indicator(s[k + 1])); }

    // A scalar inside a flow collection; *colon is set when it stopped in front of a value ':'.
    Node scalar(bool* colon) {
        ws();
        Node n;
        n.kind = Node::Scalar;
        n.line = line;
        *colon = false;
        if (i < s.size() && (s[i] == '"' || s[i] == '\'')) {
            n.scalar = scan_quoted(s, i, line);
            n.quoted = true;
            ws();
            *colon = i < s.size() && s[i] == ':';  // (behind a quoted key the ':' needs no blank)
            return n;
        }
        const size_t b = i;
        if (i < s.size() && !flow_indicator(s[i])) check_plain_start(s, i, line);
        while (i < s.size() && !flow_indicator(s[i])) {
            if (value_colon(i)) {
                *colon = true;
                break;
            }
            if (blank(s[i]) && comment_at(s, i + 1)) break;
            ++i;
        }
        n.scalar = strip(s.substr(b, i - b));
        if (n.scalar.empty()) n = Node(), n.line = line;
        return n;
    }
    Node value() {
        ws();
        if (i < s.size() && s[i] == '[') {
            ++i;
            Node n;
            n.kind = Node::List;
            n.line = line;
            for (;;) {
                ws();
                need_more("expected ',' or ']' in flow sequence");
                if (s[i] == ']') {  // (also behind a trailing comma)
                    ++i;
                    return n;
                }
                Node v = value();
                if (v.kind == Node::Null) bad(line, "empty entry in flow sequence");
                n.list.push_back(v);
                ws();
                need_more("expected ',' or ']' in flow sequence");
                if (s[i] == ',') {
                    ++i;
                    continue;
                }
                if (s[i] == ']') continue;
                if (s[i] == ':') bad(line, "a `key: value` pair inside a flow sequence is not supported (write `{key: value}`)");
                bad(line, "expected ',' or ']' in flow sequence");
            }
        }
        if (i < s.size() && s[i] == '{') {
            ++i;
            Node n;
            n.kind = Node::Map;
            n.line = line;
            for (;;) {
                ws();
                need_more("expected ',' or '}' in flow mapping");
                if (s[i] == '}') {
                    ++i;
                    return n;
                }
                if (s[i] == '[' || s[i] == '{') bad(line, "a collection as a mapping key is not supported");
                bool colon = false;
                Node k = scalar(&colon);
                if (!colon) bad(line, "expected ':' in flow mapping (a key without a value is not supported)");
                if (k.kind == Node::Null) bad(line, "empty key in flow mapping");
                ++i;
                Node v = value();
                if (n.find(k.scalar)) bad(line, "duplicate key `" + k.scalar + "` in flow mapping (also on line " + std::to_string(line) + ")");
                n.map.emplace_back(k.scalar, v);
                ws();
                need_more("expected ',' or '}' in flow mapping");
                if (s[i] == ',') {
                    ++i;
                    continue;
                }
                if (s[i] == '}') continue;
                if (s[i] == ':') bad(line, "mapping values are not allowed inside a flow-mapping value");
                bad(line, "expected ',' or '}' in flow mapping");
            }
        }
        bool colon = false;
        Node n = scalar(&colon);
        if (colon && n.quoted) return n;  // the caller reports the ':' it finds
        if (colon) bad(line, "a `key: value` pair is not allowed here (in a flow sequence write `{key: value}`)");
        return n;
    }
};

// A whole value on one line: a flow collection, a quoted scalar or a plain scalar, with an optional trailing comment.
Node parse_inline(const std::string& text, int line) {
    const std::string t = strip(text);
    Node n;
    n.line = line;
    if (t.empty() || t[0] == '#') return n;  // (the text follows a blank or opens the line: a comment)
    Flow f{t, 0, line};
    if (t[0] == '[' || t[0] == '{') {
        n = f.value();
        const size_t after = f.i;
        f.ws();
        if (f.i != t.size() || (after < t.size() && !blank(t[after]))) bad(line, "trailing characters after flow collection");
        return n;
    }
    n.kind = Node::Scalar;
    if (t[0] == '"' || t[0] == '\'') {
        n.scalar = scan_quoted(t, f.i, line);
        n.quoted = true;
        const size_t after = f.i;
        f.ws();
        if (f.i != t.size() || (after < t.size() && !blank(t[after]))) bad(line, "trailing characters after quoted scalar");
        return n;
    }
    check_plain_start(t, 0, line);
    size_t e = 0;
    for (; e < t.size(); ++e) {
        if (blank(t[e]) && comment_at(t, e + 1)) break;
        if (t[e] == ':' && (e + 1 == t.size() || blank(t[e + 1])))
            bad(line, "mapping values are not allowed here (`: ` inside a plain scalar; quote it)");
    }
    n.scalar = rstrip(t.substr(0, e));
    return n;
}

// Finds the ':' that ends a block-map key ("key: value" or "key:"); npos if the line is not a map entry.
size_t key_colon(const std::string& s, int line) {
    if (s[0] == '[' || s[0] == '{') return std::string::npos;
    if (s[0] == '"' || s[0] == '\'') {
        size_t i = 0;
        scan_quoted(s, i, line);
        while (i < s.size() && blank(s[i])) ++i;
        return (i < s.size() && s[i] == ':' && (i + 1 == s.size() || blank(s[i + 1]))) ? i : std::string::npos;
    }
    for (size_t i = 0; i < s.size(); ++i) {
        if (blank(s[i]) && comment_at(s, i + 1)) break;
        if (s[i] == ':' && (i + 1 == s.size() || blank(s[i + 1]))) return i;
    }
    return std::string::npos;
}

struct Parser {
    std::vector<Line> lines;
    size_t pos = 0;

    Node block(int indent) {
        if (pos >= lines.size()) return Node();
        const Line& first = lines[pos];
        if (is_dash_item(first.text)) return list(indent);
        if (key_colon(first.text, first.no) != std::string::npos) return map(indent);
        Node n = parse_inline(first.text, first.no);
        ++pos;
        return n;
    }

    Node list(int indent) {
        Node n;
        n.kind = Node::List;
        n.line = lines[pos].no;
        while (pos < lines.size() && lines[pos].indent == indent && is_dash_item(lines[pos].text)) {
            Line& l = lines[pos];
            std::string rest = l.text.size() > 1 ? l.text.substr(1) : std::string();
            size_t skip = 0;
            while (skip < rest.size() && rest[skip] == ' ') ++skip;
            if (skip < rest.size() && rest[skip] == '\t') bad(l.no, "tab after `-`");
            if (skip == rest.size() || rest[skip] == '#') {  // "-" alone: the item is the following deeper block
                ++pos;
                if (pos < lines.size() && lines[pos].indent > indent)
                    n.list.push_back(block(lines[pos].indent));
                else
                    n.list.push_back(Node());
            } else {
                // re-read the remainder of this line as the first line of a nested block
                l.indent = indent + 1 + int(skip);
                l.text = rest.substr(skip);
                n.list.push_back(block(l.indent));
            }
        }
        if (pos < lines.size() && lines[pos].indent > indent) bad(lines[pos].no, "unexpected indentation");
        return n;
    }

    Node map(int indent) {
        Node n;
        n.kind = Node::Map;
        n.line = lines[pos].no;
        std::vector<int> key_lines;
        while (pos < lines.size() && lines[pos].indent == indent) {
            const Line l = lines[pos];
            size_t c = key_colon(l.text, l.no);
            if (c == std::string::npos) bad(l.no, "expected 'key: value'");
            Node k = parse_inline(l.text.substr(0, c), l.no);
            if (k.kind != Node::Scalar) bad(l.no, "empty key");
            for (size_t j = 0; j < n.map.size(); ++j)
                if (n.map[j].first == k.scalar)
                    bad(l.no, "duplicate key `" + k.scalar + "` (first on line " + std::to_string(key_lines[j]) + ")");
            std::string rest = strip(l.text.substr(c + 1));
            ++pos;
            Node v;
            if (!rest.empty() && rest[0] != '#') {
                v = parse_inline(rest, l.no);
            } else if (pos < lines.size() && lines[pos].indent > indent) {
                v = block(lines[pos].indent);
            } else if (pos < lines.size() && lines[pos].indent == indent && is_dash_item(lines[pos].text)) {
                v = list(indent);  // a sequence may sit at its parent key's indentation
            }
            v.line = v.line ? v.line : l.no;
            n.map.emplace_back(k.scalar, v);
            key_lines.push_back(l.no);
        }
        if (pos < lines.size() && lines[pos].indent > indent) bad(lines[pos].no, "unexpected indentation");
        return n;
    }
};

}  // namespace

Node parse(const std::string& text) {
    Parser p;
    const bool bom = text.compare(0, 3, "\xEF\xBB\xBF") == 0;  // a UTF-8 byte order mark is no part of the first key
    p.lines = split_lines(bom ? text.substr(3) : text);
    if (p.lines.empty()) return Node();
    Node n = p.block(p.lines[0].indent);
    if (p.pos != p.lines.size()) bad(p.lines[p.pos].no, "unexpected content (indentation does not match any open block)");
    return n;
}

}  // namespace yaml_lite
