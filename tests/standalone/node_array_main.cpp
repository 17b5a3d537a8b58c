// tests/standalone/node_array_main.cpp -- TEST INFRASTRUCTURE, never part of the product and never linked into the library.
//
// A stand-alone program around the host-side pieces of the array fields of registered node types, for runs under sanitizers
// (it has its own main, so it needs nothing preloaded): the copy og_register_node takes of a description and the validation
// behind it (csrc/og_node_array_host.h, csrc/og_graph.cpp), the planes the graph compiler hands out, the look-up of a field by
// its path, the transposition between a caller's rows and the pool's planes, and the snapshot section's head -- every buffer
// an exact-size heap allocation, so that an access past an end is one the sanitizer sees.  tests/test_node_arrays_cpu.py
// builds and runs it:
//
//   clang++ -std=c++17 -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Ioscen_amd/csrc tests/standalone/node_array_main.cpp oscen_amd/csrc/og_graph.cpp oscen_amd/csrc/og_builtin.cpp \
//       -o node_array_main && ./node_array_main
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "og_abi.h"
#include "og_node_array_host.h"

namespace {
int bad = 0;
void expect(bool ok, const char* what)
{
    printf("%-96s %s\n", what, ok ? "ok" : "FAILED");
    bad += ok ? 0 : 1;
}
// 0: no exception, 1: an ogabi::Error carrying `code`, 2: any other exception
template <class F>
int thrown(F&& f, int code)
{
    try {
        f();
    } catch (const ogabi::Error& e) {
        return e.code == code ? 1 : 2;
    } catch (const std::exception&) {
        return 2;
    }
    return 0;
}
char* heap_str(const char* s)
{
    char* p = (char*)malloc(strlen(s) + 1);
    memcpy(p, s, strlen(s) + 1);
    return p;
}
uint32_t* heap_words(size_t n, uint32_t fill)
{
    uint32_t* p = (uint32_t*)malloc(n ? n * 4 : 1);
    for (size_t i = 0; i < n; ++i) p[i] = fill;
    return p;
}

ogc::UserNodeType comb_type(const char* name, std::vector<ogc::UserArray> arrays)
{
    ogc::UserNodeType u;
    u.type = name;
    u.inputs.push_back({"input", ogc::Kind::Stream, 0.0f, -1, 1});
    u.outputs.push_back("output");
    ogc::UserState wp;
    wp.name = "wp";
    wp.is_uint = true;
    u.state.push_back(wp);
    u.arrays = std::move(arrays);
    u.process_src = "    output = input;\n";
    return u;
}
ogc::UserArray arr(const char* name, uint32_t length, bool is_uint = false)
{
    ogc::UserArray a;
    a.name = name;
    a.length = length;
    a.is_uint = is_uint;
    a.init_f = 0.5f;
    a.init_u = 7u;
    return a;
}
ogc::GraphDesc graph_of(const std::vector<ogc::GNode>& nodes)
{
    ogc::GraphDesc g;
    g.name = "narr_host";
    ogc::GOutput out;
    out.name = "out";
    g.outputs.push_back(out);
    g.nodes.push_back({"osc", "PolyBlepOscillator::saw", {220.0f, 0.3f}});
    for (const ogc::GNode& n : nodes) {
        g.nodes.push_back(n);
        g.edges.push_back({"osc.output", n.name + ".input", "", false});
        if (!n.array_len) {
            g.edges.push_back({n.name + ".output", "out", "", false});
        } else { // (an array's fan-in sum takes an input of its own)
            g.nodes.push_back({"sum_" + n.name, "HSum::new", {}});
            g.edges.push_back({n.name + ".output", "sum_" + n.name + ".input", "", false});
            g.edges.push_back({"sum_" + n.name + ".output", "out", "", false});
        }
    }
    return g;
}
ogc::GNode node(const char* name, const char* type, uint32_t array_len = 0)
{
    ogc::GNode n;
    n.name = name;
    n.type = type;
    n.array_len = array_len;
    return n;
}
} // namespace

int main()
{
    // ---- the copy of a description ------------------------------------------------------------------------------------------
    {
        og_node_array* d = (og_node_array*)malloc(2 * sizeof(og_node_array));
        char *n0 = heap_str("buf"), *n1 = heap_str("ids");
        d[0] = og_node_array{n0, 1024u, 0, 0.25f, 0u};
        d[1] = og_node_array{n1, 3u, 1, 0.0f, 9u};
        std::vector<ogc::UserArray> out;
        ognarr::copy_arrays(d, 2, out);
        memset(n0, 'x', 3);
        free(n0);
        free(n1);
        free(d);
        expect(out.size() == 2 && out[0].name == "buf" && out[0].length == 1024u && !out[0].is_uint && out[0].init_f == 0.25f && out[1].name == "ids" &&
                   out[1].is_uint && out[1].init_u == 9u,
               "copy_arrays: names and values are the library's own once the call returns");
        std::vector<ogc::UserArray> none;
        ognarr::copy_arrays(nullptr, 0, none);
        expect(none.empty(), "copy_arrays: no arrays");
        expect(thrown([&] { ognarr::copy_arrays(nullptr, 1, none); }, 0) == 2, "copy_arrays: n_arrays > 0 with a null pointer");
        og_node_array nameless{nullptr, 4u, 0, 0.0f, 0u};
        expect(thrown([&] { ognarr::copy_arrays(&nameless, 1, none); }, 0) == 2, "copy_arrays: a null name");
        std::vector<og_node_array> nine(9, og_node_array{"a", 1u, 0, 0.0f, 0u});
        expect(thrown([&] { ognarr::copy_arrays(nine.data(), 9, none); }, 0) == 2 && none.empty(), "copy_arrays: nine arrays");
    }
    // ---- validation ---------------------------------------------------------------------------------------------------------
    expect(thrown([] { ogc::register_user_node(comb_type("HComb::new", {arr("buf", 1024), arr("tab", 65536, true)})); }, 0) == 0, "register: accepted");
    expect(thrown([] { ogc::register_user_node(comb_type("HBad::new", {arr("buf", 4), arr("buf", 4)})); }, 0) == 2, "register: duplicate array name");
    expect(thrown([] { ogc::register_user_node(comb_type("HBad::new", {arr("wp", 4)})); }, 0) == 2, "register: array named like a state field");
    expect(thrown([] { ogc::register_user_node(comb_type("HBad::new", {arr("input", 4)})); }, 0) == 2, "register: array named like an input");
    expect(thrown([] { ogc::register_user_node(comb_type("HBad::new", {arr("1st", 4)})); }, 0) == 2, "register: not an identifier");
    expect(thrown([] { ogc::register_user_node(comb_type("HBad::new", {arr("buf", 0)})); }, 0) == 2, "register: length 0");
    expect(thrown([] { ogc::register_user_node(comb_type("HBad::new", {arr("buf", 65537)})); }, OG_E_UNSUPPORTED) == 1, "register: length above the limit is OG_E_UNSUPPORTED");
    expect(thrown([] { ogc::register_user_node(comb_type("HBad::new", std::vector<ogc::UserArray>(9, arr("a", 1)))); }, 0) == 2, "register: nine arrays");
    ogc::register_user_node(comb_type("HSum::new", {}));
    // ---- planes -------------------------------------------------------------------------------------------------------------
    ogc::register_user_node(comb_type("HLine::new", {arr("buf", 1024), arr("ids", 3, true)}));
    {
        const auto cg = ogc::compile(graph_of({node("a", "HLine::new"), node("combs", "HLine::new", 3), node("b", "HLine::new")}));
        const auto& f = cg->arrays;
        bool ok = f.size() == 10 && cg->narr_slot0 >= 0 && cg->array_words() == 5 * 1027u;
        for (size_t k = 0; ok && k < f.size(); ++k) {
            ok = f[k].base == (k ? f[k - 1].base + f[k - 1].length : 0u) && f[k].length == (k % 2 ? 3u : 1024u) && f[k].is_uint == (k % 2 == 1);
            ok = ok && f[k].init == (k % 2 ? 7u : 0x3F000000u);
        }
        expect(ok, "compile: every (instance, field) has its own planes, back to back, with its init bits");
        auto is = [&](const char* path, const char* flat, uint32_t length) { // (the planes follow the schedule, not the declarations)
            const int k = ognarr::find_field(f, path);
            return k >= 0 && f[k].path == flat && f[k].length == length;
        };
        expect(is("a.buf", "a.buf", 1024) && is("combs[1].ids", "combs__1.ids", 3) && is(" combs[2].buf", "combs__2.buf", 1024) && is("b.ids", "b.ids", 3),
               "find_field: instances and elements of a node array");
        expect(ognarr::find_field(f, "a.wp") == -1 && ognarr::find_field(f, "combs.buf") == -1 && ognarr::find_field(f, "combs[3].buf") == -1 &&
                   ognarr::find_field(f, "") == -1 && ognarr::find_field(f, "osc.buf") == -1,
               "find_field: scalar fields, whole arrays of nodes, elements past the end");
        expect(ognarr::pool_bytes(f, 70) == (uint64_t)5 * 1027 * 70 * 4 && ognarr::pool_bytes(f, 0xFFFFFFFFu) > ((uint64_t)1 << 44), "pool_bytes: 64-bit");
        expect(cg->source.find("#include \"og_node_array.hip.h\"") != std::string::npos, "compile: the unit includes og_node_array.hip.h");
    }
    {
        const auto cg = ogc::compile(graph_of({}));
        expect(cg->arrays.empty() && cg->narr_slot0 < 0 && cg->source.find("og_node_array") == std::string::npos && ognarr::section_head_bytes(cg->arrays) == 0,
               "compile: a graph without array fields knows nothing of the header");
    }
    {
        std::vector<ogc::GNode> many;
        static char names[16][8];
        for (int k = 0; k < 16; ++k) {
            snprintf(names[k], sizeof names[k], "t%d", k);
            many.push_back(node(names[k], "HComb::new"));
        }
        expect(thrown([&] { (void)ogc::compile(graph_of(many)); }, OG_E_UNSUPPORTED) == 1, "compile: more than 2^20 array words per voice is OG_E_UNSUPPORTED");
        many.resize(15);
        expect(thrown([&] { (void)ogc::compile(graph_of(many)); }, 0) == 0, "compile: 15 x (1024 + 65536) words fit");
    }
    // ---- rows <-> planes ----------------------------------------------------------------------------------------------------
    {
        ognarr::Field f;
        f.length = 5;
        const uint32_t V = 7;
        uint32_t* planes = heap_words((size_t)f.length * V, 0xAAAAAAAAu);
        uint32_t* rows = heap_words((size_t)3 * f.length, 0u);
        for (uint32_t i = 0; i < 15; ++i) rows[i] = 100 + i;
        const uint32_t rev[7] = {6, 5, 4, 3, 2, 1, 0};
        ognarr::scatter_rows(f, V, nullptr, 4, 3, rows, planes); // the last three voices
        bool ok = true;
        for (uint32_t i = 0; i < 5; ++i)
            for (uint32_t v = 0; v < V; ++v) ok = ok && planes[i * V + v] == (v >= 4 ? 100 + (v - 4) * 5 + i : 0xAAAAAAAAu);
        expect(ok, "scatter_rows: a range at the end of the bank, nothing else touched");
        uint32_t* back = heap_words(15, 0u);
        ognarr::gather_rows(f, V, nullptr, 4, 3, planes, back);
        expect(memcmp(back, rows, 60) == 0, "gather_rows: the same rows back");
        ognarr::scatter_rows(f, V, rev, 0, 3, rows, planes); // logical 0..2 -> slots 6, 5, 4
        ognarr::gather_rows(f, V, rev, 0, 3, planes, back);
        expect(memcmp(back, rows, 60) == 0 && planes[0 * V + 6] == 100 && planes[4 * V + 4] == 114, "scatter / gather through a voice -> slot map");
        ognarr::gather_rows(f, V, nullptr, 7, 0, planes, back);
        free(planes);
        free(rows);
        free(back);
    }
    // ---- the snapshot section's head ----------------------------------------------------------------------------------------
    {
        std::vector<ognarr::Field> f(3);
        f[0].path = "a.buf", f[0].base = 0, f[0].length = 1024;
        f[1].path = "a.ids", f[1].base = 1024, f[1].length = 3, f[1].is_uint = true;
        f[2].path = "b.buf", f[2].base = 1027, f[2].length = 1;
        const size_t n = ognarr::section_head_bytes(f);
        char* head = (char*)malloc(n);
        ognarr::write_section_head(f, head);
        expect(n == 20 && ognarr::check_section_head(f, head, n).empty() && ognarr::check_section_head(f, head, n + 1000).empty(), "section head: written and accepted");
        bool all = true;
        for (size_t cut = 0; cut < n; ++cut) { // every truncation, each in an allocation of exactly that size
            char* part = (char*)malloc(cut ? cut : 1);
            memcpy(part, head, cut);
            all = all && !ognarr::check_section_head(f, part, cut).empty();
            free(part);
        }
        expect(all, "section head: every truncation is refused without reading past it");
        auto g = f;
        g[2].length = 2;
        expect(ognarr::check_section_head(g, head, n).find("b.buf") != std::string::npos, "section head: another length names the field");
        g = f;
        g[1].is_uint = false;
        expect(!ognarr::check_section_head(g, head, n).empty(), "section head: another element type");
        g = f;
        g.pop_back();
        expect(ognarr::check_section_head(g, head, n).find("3 node-array fields") != std::string::npos, "section head: another field count");
        uint32_t huge[2] = {ognarr::SNAP_NARR_MAGIC, 0xFFFFFFFFu};
        expect(!ognarr::check_section_head(f, huge, sizeof huge).empty(), "section head: a crafted count");
        head[0] ^= 1;
        expect(!ognarr::check_section_head(f, head, n).empty(), "section head: another magic");
        expect(ognarr::check_section_head({}, nullptr, 0).empty(), "section head: graphs without array fields have none");
        free(head);
    }
    ogc::unregister_user_node("HComb::new");
    ogc::unregister_user_node("HLine::new");
    ogc::unregister_user_node("HSum::new");
    printf(bad ? "%d node-array case(s) FAILED\n" : "all node-array host cases as expected\n", bad);
    return bad ? 1 : 0;
}
