// meshuv_kat_main.cpp — known-answer tests of the OBJ parser's texture coordinates, at the level
// where a line error is visible: ObjParser::lines_ignored and ignored_by_error of the PRODUCT host library.  A line error
// never leaves the parser (obj.zig:277), so "refused by name" is the name the line was counted under.
// Output format is host_kat_main.cpp's: "KAT <where> <name> PASS|FAIL".
#include <cstdio>
#include <string>

#include "../../ray-tracer-challenge_amd/host/rtc_loader.hpp"

using namespace rtc;

static int g_failed = 0, g_total = 0;
static void report(const char* where, const std::string& name, bool ok, const std::string& detail = "") {
  ++g_total;
  if (!ok) ++g_failed;
  std::printf("KAT %s %s %s%s%s\n", where, name.c_str(), ok ? "PASS" : "FAIL", detail.empty() ? "" : " ", detail.c_str());
}
static size_t by(const ObjParser& p, const char* name) {
  const auto it = p.ignored_by_error.find(name);
  return it == p.ignored_by_error.end() ? 0 : it->second;
}

// Three vertices and normals, a comment, `vt` lines of every sort - one number, three numbers, no number, two numbers - and
// faces whose t fields point nowhere (the second is obj.zig:511's).
static const char* kVertices =
    "# a comment\nv 0 1 0\nvt 0.5\nv -1 0 0\nvt 1 2 3\nv 1 0 0\nvn -1 0 0\nvn 1 0 0\nvn 0 1 0\nvt x y\nvt 0.25 0.75\n";
static const char* kJunkFaces = "f 1/0 2/102 3/14\nf 1/0/3 2/102/1 3/14/2\n";

int main() {
  {  // the key absent (the parser's default): what the parser did before it knew `vt` - the comment and every one of the
     // four `vt` lines is an ignored line under UnknownFirstToken, the junk t fields are never read, both faces load
    ObjParser p;
    p.loadObj(std::string(kVertices) + kJunkFaces, {}, false);
    const auto& c = p.default_group.children;
    report("meshuv", "key_absent_lines_ignored", p.lines_ignored == 5, std::to_string(p.lines_ignored));
    report("meshuv", "key_absent_every_vt_is_an_unknown_first_token", by(p, "UnknownFirstToken") == 5 && p.ignored_by_error.size() == 1);
    bool ok = c.size() == 2 && c[0].kind == ShapeKind::Triangle && c[1].kind == ShapeKind::SmoothTriangle && p.texcoords.empty();
    for (size_t i = 0; ok && i < c.size(); ++i)
      for (int k = 0; k < 6; ++k) ok = ok && c[i].tex_uv[k] == 0.0;
    report("meshuv", "key_absent_faces_load_without_rows", ok);
  }
  {  // the same text without any `vt` line: four ignored lines fewer, the same triangles
    ObjParser p, q;
    p.loadObj(std::string("# a comment\nv 0 1 0\nv -1 0 0\nv 1 0 0\nvn -1 0 0\nvn 1 0 0\nvn 0 1 0\n") + kJunkFaces, {}, false);
    q.loadObj(std::string(kVertices) + kJunkFaces, {}, false);
    bool ok = p.lines_ignored == 1 && p.default_group.children.size() == q.default_group.children.size();
    for (size_t i = 0; ok && i < p.default_group.children.size(); ++i) {
      const Shape &a = p.default_group.children[i], &b = q.default_group.children[i];
      ok = a.kind == b.kind && a.p1.bitEqual(b.p1) && a.p2.bitEqual(b.p2) && a.p3.bitEqual(b.p3) && a.n1.bitEqual(b.n1) &&
           a.n2.bitEqual(b.n2) && a.n3.bitEqual(b.n3);
    }
    report("meshuv", "vt_lines_change_no_triangle_without_the_key", ok);
  }
  {  // the key set: `vt 0.5` is IncompleteVertex, `vt x y` InvalidCharacter, `vt 1e999 0` NonFiniteVertex, the comment
     // UnknownFirstToken; `vt 1 2 3` (w not read) and `vt 0.25 0.75` are the list
    ObjParser p;
    p.texture_coordinates = true;
    p.loadObj(std::string(kVertices) + "vt 1e999 0\nf 1/1 2/2 3\n", {}, false);
    report("meshuv", "key_set_lines_ignored", p.lines_ignored == 4, std::to_string(p.lines_ignored));
    report("meshuv", "vt_with_one_number_is_IncompleteVertex", by(p, "IncompleteVertex") == 1);
    report("meshuv", "vt_without_a_number_is_InvalidCharacter", by(p, "InvalidCharacter") == 1);
    report("meshuv", "vt_not_finite_is_NonFiniteVertex", by(p, "NonFiniteVertex") == 1);
    report("meshuv", "comment_is_UnknownFirstToken", by(p, "UnknownFirstToken") == 1 && p.ignored_by_error.size() == 4);
    const auto& c = p.default_group.children;
    const double want[6] = {1.0, 2.0, 0.25, 0.75, 0.0, 0.0};
    bool ok = p.texcoords.size() == 2 && c.size() == 1;
    for (int k = 0; ok && k < 6; ++k) ok = c[0].tex_uv[k] == want[k];
    report("meshuv", "key_set_rows", ok);
  }
  {  // a `vt` alone on its line has no first number either
    ObjParser p;
    p.texture_coordinates = true;
    p.loadObj("vt\nvt 1\n", {}, false);
    report("meshuv", "vt_alone_is_IncompleteVertex", p.lines_ignored == 2 && by(p, "IncompleteVertex") == 2 && p.texcoords.empty());
  }
  {  // the key set and a t field out of range: not a line error - the load fails, naming the texture index
    ObjParser p;
    p.texture_coordinates = true;
    std::string name, detail;
    try {
      p.loadObj(std::string(kVertices) + kJunkFaces, {}, false);
    } catch (const Error& e) {
      name = e.name;
      detail = e.what();
    }
    report("meshuv", "t_out_of_range_is_IndexOutOfBounds", name == "IndexOutOfBounds" && detail.find("texture 0") != std::string::npos, detail);
  }
  std::printf("KAT summary: %d/%d passed\n", g_total - g_failed, g_total);
  return g_failed ? 1 : 0;
}
