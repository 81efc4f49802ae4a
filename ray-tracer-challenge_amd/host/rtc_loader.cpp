// rtc_loader.cpp — scene JSON + OBJ loading.
//
// Restated from the reference (quirks listed in SURVEY §3.3 are kept on purpose:
// they fix leaf matrices, leaf order and group boxes, i.e. the kernel's input):
//   scene.zig:164-190   ObjectConfig.inherit (own transform applied AFTER the inherited one)
//   scene.zig:214-241   parseTransform (list order, each op left-multiplies)
//   scene.zig:300-405   parsePattern
//   scene.zig:407-430   parseMaterial (override-merge on the inherited material)
//   scene.zig:440-591   parseObject (from-definition double inherit, group children
//                       parsed with identity transform, setTransform, divide(8))
//   scene.zig:593-661   parseLight, parseScene
//   obj.zig:53-283      ObjParser
#include "rtc_loader.hpp"

#include "../../include/rtc.h"

#include <sched.h>
#include <zlib.h>

#include <atomic>
#include <cerrno>
#include <cstdio>
#include <exception>
#include <system_error>
#include <thread>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>

#include "rtc_json.hpp"

namespace rtc {

using json::Value;

FileLoader directoryLoader(const std::string& dir) {
  return [dir](const std::string& name) {
    const std::string path = dir.empty() ? name : dir + "/" + name;
    std::ifstream f(path, std::ios::binary);
    if (!f) throw Error("FileNotFound", path);
    std::ostringstream ss;
    ss << f.rdbuf();
    return ss.str();
  };
}

namespace {

// ---- typed access with std.json-style errors -------------------------------------------
const Value& requireObject(const Value& v, const char* what) {
  if (v.type != Value::Object) throw Error("UnexpectedToken", std::string("expected object for ") + what);
  return v;
}
const Value& requireArray(const Value& v, const char* what) {
  if (v.type != Value::Array) throw Error("UnexpectedToken", std::string("expected array for ") + what);
  return v;
}
double asFloat(const Value& v, const char* what) {
  if (v.type != Value::Number) throw Error("UnexpectedToken", std::string("expected number for ") + what);
  return v.num;
}
size_t asUsize(const Value& v, const char* what) {
  if (v.type != Value::Number) throw Error("UnexpectedToken", std::string("expected integer for ") + what);
  if (v.num < 0) throw Error("Overflow", what);
  const double r = std::floor(v.num);
  if (r != v.num) throw Error("InvalidNumber", what);
  return static_cast<size_t>(r);
}
bool asBool(const Value& v, const char* what) {
  if (v.type != Value::Bool) throw Error("UnexpectedToken", std::string("expected bool for ") + what);
  return v.b;
}
const std::string& asString(const Value& v, const char* what) {
  if (v.type != Value::String) throw Error("UnexpectedToken", std::string("expected string for ") + what);
  return v.str;
}
void asVec3(const Value& v, const char* what, double out[3]) {
  requireArray(v, what);
  if (v.arr.size() != 3) throw Error("LengthMismatch", what);
  for (int i = 0; i < 3; ++i) out[i] = asFloat(v.arr[i], what);
}
// Checks an object against its allowed field list: duplicates and unknown names are
// errors (std.json defaults: duplicate_field_behavior=.error, ignore_unknown_fields=false).
void checkFields(const Value& obj, std::initializer_list<const char*> allowed, const char* what) {
  for (size_t i = 0; i < obj.obj.size(); ++i) {
    const std::string& k = obj.obj[i].first;
    bool ok = false;
    for (const char* a : allowed) ok = ok || k == a;
    if (!ok) throw Error("UnknownField", std::string(what) + "." + k);
    for (size_t j = 0; j < i; ++j)
      if (obj.obj[j].first == k) throw Error("DuplicateField", std::string(what) + "." + k);
  }
}
const Value& requireField(const Value& obj, const char* key, const char* what) {
  const Value* v = obj.find(key);
  if (!v) throw Error("MissingField", std::string(what) + "." + key);
  return *v;
}
// A Zig union(enum) is encoded as an object with exactly one member.
const std::pair<std::string, Value>& unionMember(const Value& v, const char* what) {
  requireObject(v, what);
  if (v.obj.size() != 1) throw Error("UnexpectedToken", std::string("union ") + what + " needs exactly one member");
  return v.obj[0];
}
void requireVoid(const Value& v, const char* what) {  // `sphere: void` is written {}
  if (v.type != Value::Object || !v.obj.empty()) throw Error("UnexpectedToken", std::string("expected {} for ") + what);
}

// ---- scene.zig:214-241 ------------------------------------------------------------------
Matrix4 parseTransform(const Value& list) {
  requireArray(list, "transform");
  Matrix4 m = Matrix4::identity();
  for (const Value& item : list.arr) {
    const auto& kv = unionMember(item, "transform entry");
    const std::string& op = kv.first;
    if (op == "translate" || op == "scale") {
      double b[3];
      asVec3(kv.second, op.c_str(), b);
      m = (op == "translate") ? m.translate(b[0], b[1], b[2]) : m.scale(b[0], b[1], b[2]);
    } else if (op == "rotate-x") {
      m = m.rotateX(asFloat(kv.second, "rotate-x"));
    } else if (op == "rotate-y") {
      m = m.rotateY(asFloat(kv.second, "rotate-y"));
    } else if (op == "rotate-z") {
      m = m.rotateZ(asFloat(kv.second, "rotate-z"));
    } else if (op == "shear") {
      const Value& o = requireObject(kv.second, "shear");
      checkFields(o, {"xy", "xz", "yx", "yz", "zx", "zy"}, "shear");
      ShearArgs a;
      if (auto* v = o.find("xy")) a.xy = asFloat(*v, "xy");
      if (auto* v = o.find("xz")) a.xz = asFloat(*v, "xz");
      if (auto* v = o.find("yx")) a.yx = asFloat(*v, "yx");
      if (auto* v = o.find("yz")) a.yz = asFloat(*v, "yz");
      if (auto* v = o.find("zx")) a.zx = asFloat(*v, "zx");
      if (auto* v = o.find("zy")) a.zy = asFloat(*v, "zy");
      m = m.shear(a);
    } else {
      throw Error("UnknownField", "transform." + op);
    }
  }
  return m;
}

// ---- scene.zig:300-405 ------------------------------------------------------------------
// A PNG as zigimg hands it to Canvas.fromImage (scene.zig:282-285, canvas.zig:34-46): every pixel as an f32
// colour, channel / max (zigimg color.zig toF32Color; the pinned zigimg is not in the tree).  Supports what
// the reference's data files are and a little more: non-interlaced, 8 or 16 bits, grey / RGB / palette /
// with alpha (dropped: canvas.zig:41 keeps r, g, b).
UvImageData decodePng(const std::string& bytes) {
  auto be32 = [&](size_t off) {
    return (static_cast<uint32_t>(static_cast<unsigned char>(bytes[off])) << 24) |
           (static_cast<uint32_t>(static_cast<unsigned char>(bytes[off + 1])) << 16) |
           (static_cast<uint32_t>(static_cast<unsigned char>(bytes[off + 2])) << 8) |
           static_cast<uint32_t>(static_cast<unsigned char>(bytes[off + 3]));
  };
  static const unsigned char kSig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  if (bytes.size() < 8 + 25 || std::memcmp(bytes.data(), kSig, 8) != 0)
    throw Error("Unsupported", "image: not a PNG (the reference decodes other formats through zigimg)");
  uint32_t width = 0, height = 0;
  unsigned depth = 0, color = 0, interlace = 0;
  std::string idat;
  std::vector<unsigned char> palette;
  size_t off = 8;
  bool seen_ihdr = false, seen_iend = false;
  while (off + 12 <= bytes.size() && !seen_iend) {
    const uint32_t len = be32(off);
    const std::string type = bytes.substr(off + 4, 4);
    if (off + 12 + static_cast<size_t>(len) > bytes.size()) throw Error("EndOfStream", "png chunk " + type);
    const size_t data = off + 8;
    if (type == "IHDR") {
      if (len != 13) throw Error("InvalidData", "png IHDR");
      width = be32(data);
      height = be32(data + 4);
      depth = static_cast<unsigned char>(bytes[data + 8]);
      color = static_cast<unsigned char>(bytes[data + 9]);
      interlace = static_cast<unsigned char>(bytes[data + 12]);
      seen_ihdr = true;
    } else if (type == "PLTE") {
      palette.assign(bytes.begin() + data, bytes.begin() + data + len);
    } else if (type == "IDAT") {
      idat.append(bytes, data, len);
    } else if (type == "IEND") {
      seen_iend = true;
    }
    off += 12 + static_cast<size_t>(len);
  }
  if (!seen_ihdr || width == 0 || height == 0) throw Error("InvalidData", "png without IHDR");
  if (interlace != 0) throw Error("Unsupported", "interlaced png");
  if (depth != 8 && depth != 16) throw Error("Unsupported", "png bit depth " + std::to_string(depth));
  unsigned channels = 0;
  switch (color) {
    case 0: channels = 1; break;
    case 2: channels = 3; break;
    case 3: channels = 1; break;
    case 4: channels = 2; break;
    case 6: channels = 4; break;
    default: throw Error("InvalidData", "png colour type");
  }
  if (color == 3 && depth != 8) throw Error("Unsupported", "png palette depth");
  const size_t bpp = channels * (depth / 8), stride = static_cast<size_t>(width) * bpp;
  std::vector<unsigned char> raw((stride + 1) * height);
  uLongf out_len = static_cast<uLongf>(raw.size());
  if (uncompress(raw.data(), &out_len, reinterpret_cast<const Bytef*>(idat.data()), static_cast<uLong>(idat.size())) != Z_OK ||
      out_len != raw.size())
    throw Error("InvalidData", "png IDAT does not inflate to the image size");
  // undo the scanline filters (PNG spec 9.2)
  std::vector<unsigned char> img(stride * height);
  for (uint32_t y = 0; y < height; ++y) {
    const unsigned char filter = raw[(stride + 1) * y];
    const unsigned char* in = &raw[(stride + 1) * y + 1];
    unsigned char* cur = &img[stride * y];
    const unsigned char* up = y ? &img[stride * (y - 1)] : nullptr;
    for (size_t i = 0; i < stride; ++i) {
      const int a = i >= bpp ? cur[i - bpp] : 0, b = up ? up[i] : 0, c = (up && i >= bpp) ? up[i - bpp] : 0;
      int pred = 0;
      switch (filter) {
        case 0: pred = 0; break;
        case 1: pred = a; break;
        case 2: pred = b; break;
        case 3: pred = (a + b) / 2; break;
        case 4: {
          const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
          pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
          break;
        }
        default: throw Error("InvalidData", "png filter type");
      }
      cur[i] = static_cast<unsigned char>(in[i] + pred);
    }
  }
  UvImageData out;
  out.width = width;
  out.height = height;
  out.rgb.resize(static_cast<size_t>(width) * height * 3);
  auto sample = [&](const unsigned char* p) {  // one channel as zigimg's toF32Color
    return depth == 8 ? static_cast<float>(p[0]) / 255.0f : static_cast<float>((p[0] << 8) | p[1]) / 65535.0f;
  };
  for (size_t i = 0; i < static_cast<size_t>(width) * height; ++i) {
    const unsigned char* px = &img[i * bpp];
    float r, g, b;
    if (color == 3) {
      const size_t k = px[0];
      if (3 * k + 2 >= palette.size()) throw Error("InvalidData", "png palette index");
      r = static_cast<float>(palette[3 * k]) / 255.0f;
      g = static_cast<float>(palette[3 * k + 1]) / 255.0f;
      b = static_cast<float>(palette[3 * k + 2]) / 255.0f;
    } else if (channels <= 2) {
      r = g = b = sample(px);
    } else {
      r = sample(px);
      g = sample(px + depth / 8);
      b = sample(px + 2 * (depth / 8));
    }
    out.rgb[3 * i] = r;
    out.rgb[3 * i + 1] = g;
    out.rgb[3 * i + 2] = b;
  }
  return out;
}

Pattern parsePattern(const Value& cfg, const FileLoader& load_file_data);

// scene.zig:243-298
UvPattern parseUvPattern(const Value& cfg, const FileLoader& load_file_data) {
  const auto& kv = unionMember(cfg, "uv-pattern");
  const std::string& t = kv.first;
  UvPattern uv;
  auto sub = [&](const Value& v) { return std::make_shared<const Pattern>(parsePattern(v, load_file_data)); };
  if (t == "align-check") {
    requireObject(kv.second, "align-check");
    checkFields(kv.second, {"central", "upper-left", "upper-right", "bottom-left", "bottom-right"}, "align-check");
    uv.kind = UvKind::AlignCheck;
    for (const char* f : {"central", "upper-left", "upper-right", "bottom-left", "bottom-right"})
      uv.sub.push_back(sub(requireField(kv.second, f, "align-check")));
  } else if (t == "checkers") {
    requireObject(kv.second, "uv checkers");
    checkFields(kv.second, {"width", "height", "patterns"}, "uv checkers");
    uv.kind = UvKind::Checkers;
    uv.width = asFloat(requireField(kv.second, "width", "uv checkers"), "width");
    uv.height = asFloat(requireField(kv.second, "height", "uv checkers"), "height");
    const Value& ps = requireField(kv.second, "patterns", "uv checkers");
    requireArray(ps, "patterns");
    if (ps.arr.size() != 2) throw Error("LengthMismatch", "uv checkers patterns");
    uv.sub.push_back(sub(ps.arr[0]));
    uv.sub.push_back(sub(ps.arr[1]));
  } else if (t == "image") {
    requireObject(kv.second, "image");
    checkFields(kv.second, {"file", "interpolation"}, "image");
    uv.kind = UvKind::Image;
    const std::string& file = asString(requireField(kv.second, "file", "image"), "file");
    if (const Value* ip = kv.second.find("interpolation")) {
      const std::string& mode = asString(*ip, "interpolation");
      if (mode == "bilinear") {
        uv.bilinear = true;
      } else if (mode != "none") {
        throw Error("InvalidEnumTag", "image.interpolation " + mode);
      }
    }
    uv.image = std::make_shared<const UvImageData>(decodePng(load_file_data(file)));
  } else if (t == "test") {  // UvTestPattern (texture_map.zig:13-17): colour = (u, v, 0); the reference's scene files cannot name it
    requireObject(kv.second, "test");
    checkFields(kv.second, {}, "test");
    uv.kind = UvKind::Test;
  } else {
    throw Error("UnknownField", "uv-pattern." + t);
  }
  return uv;
}

Pattern parsePattern(const Value& cfg, const FileLoader& load_file_data) {
  requireObject(cfg, "pattern");
  checkFields(cfg, {"type", "transform"}, "pattern");
  const auto& kv = unionMember(requireField(cfg, "type", "pattern"), "pattern.type");
  const std::string& t = kv.first;
  Pattern pat;
  auto two = [&](PatternKind k) {
    requireArray(kv.second, t.c_str());
    if (kv.second.arr.size() != 2) throw Error("LengthMismatch", t);
    return Pattern::binary(k, parsePattern(kv.second.arr[0], load_file_data), parsePattern(kv.second.arr[1], load_file_data));
  };
  if (t == "solid") {
    double c[3];
    asVec3(kv.second, "solid", c);
    pat = Pattern::solid({c[0], c[1], c[2]});
  } else if (t == "stripes") {
    pat = two(PatternKind::Stripes);
  } else if (t == "rings") {
    pat = two(PatternKind::Rings);
  } else if (t == "gradient") {
    pat = two(PatternKind::Gradient);
  } else if (t == "radial-gradient") {
    pat = two(PatternKind::RadialGradient);
  } else if (t == "checkers") {
    pat = two(PatternKind::Checkers);
  } else if (t == "blend") {
    pat = two(PatternKind::Blend);
  } else if (t == "perturb") {
    pat.kind = PatternKind::Perturb;
    pat.a = std::make_shared<const Pattern>(parsePattern(kv.second, load_file_data));
  } else if (t == "texture-map") {  // scene.zig:366-396
    const auto& mk = unionMember(kv.second, "texture-map");
    TextureMap tm;
    auto single = [&](TexMapping m) {
      requireObject(mk.second, mk.first.c_str());
      checkFields(mk.second, {"uv-pattern"}, mk.first.c_str());
      tm.mapping = m;
      tm.faces.push_back(parseUvPattern(requireField(mk.second, "uv-pattern", mk.first.c_str()), load_file_data));
    };
    if (mk.first == "spherical") {
      single(TexMapping::Spherical);
    } else if (mk.first == "planar") {
      single(TexMapping::Planar);
    } else if (mk.first == "cylindrical") {
      single(TexMapping::Cylindrical);
    } else if (mk.first == "mesh") {  // (not in the reference): (u, v) from the hit triangle's texture row
      single(TexMapping::Mesh);
    } else if (mk.first == "cubic") {
      requireObject(mk.second, "cubic");
      checkFields(mk.second, {"front", "back", "left", "right", "up", "down"}, "cubic");
      tm.mapping = TexMapping::Cubic;
      for (const char* f : {"front", "back", "left", "right", "up", "down"})  // scene.zig:387-393, Cubic.Face order
        tm.faces.push_back(parseUvPattern(requireField(mk.second, f, "cubic"), load_file_data));
    } else {
      throw Error("UnknownField", "texture-map." + mk.first);
    }
    pat.kind = PatternKind::TextureMap;
    pat.texture_map = std::make_shared<const TextureMap>(std::move(tm));
  } else {
    throw Error("UnknownField", "pattern.type." + t);
  }
  if (const Value* tr = cfg.find("transform")) {
    if (tr->type != Value::Null) pat.setTransform(parseTransform(*tr));
  }
  return pat;
}

// Whether a texture map of mapping "mesh" sits anywhere in a pattern: below a select, a mix or a perturb, or among a uv
// pattern's sub-patterns (the environment's pattern, DESIGN.md section 24, has no triangle to read a texture row from).
bool hasMeshMap(const Pattern& p) {
  if (p.kind == PatternKind::TextureMap && p.texture_map) {
    if (p.texture_map->mapping == TexMapping::Mesh) return true;
    for (const UvPattern& uv : p.texture_map->faces)
      for (const auto& sub : uv.sub)
        if (sub && hasMeshMap(*sub)) return true;
  }
  return (p.a && hasMeshMap(*p.a)) || (p.b && hasMeshMap(*p.b));
}

// ---- scene.zig:407-430 ------------------------------------------------------------------
const Value* presentField(const Value& obj, const char* k) {
  const Value* v = obj.find(k);
  return (v && v->type != Value::Null) ? v : nullptr;
}

// A material's "normal-perturbation" (not in the reference): {"type": "noise" | "ripples",
// "amplitude": a, "octaves": n, "persistence": p, "transform": [...]}, the transform list as a pattern's.
Bump parseBump(const Value& cfg) {
  const char* what = "normal-perturbation";
  requireObject(cfg, what);
  checkFields(cfg, {"type", "amplitude", "octaves", "persistence", "transform"}, what);
  Bump b;
  const std::string& t = asString(requireField(cfg, "type", what), "normal-perturbation.type");
  if (t == "noise") {
    b.kind = RTC_BUMP_NOISE;
  } else if (t == "ripples") {
    b.kind = RTC_BUMP_RIPPLES;
  } else {
    throw Error("UnknownField", "normal-perturbation.type." + t);
  }
  b.amplitude = asFloat(requireField(cfg, "amplitude", what), "normal-perturbation.amplitude");
  if (!(std::isfinite(b.amplitude) && b.amplitude >= 0.0)) throw Error("InvalidData", "normal-perturbation.amplitude: a finite number, 0 or above");
  if (const Value* v = presentField(cfg, "octaves")) {
    if (b.kind != RTC_BUMP_NOISE) throw Error("InvalidData", "normal-perturbation.octaves: of \"noise\" only");
    const size_t n = asUsize(*v, "normal-perturbation.octaves");
    if (n == 0 || n > RTC_BUMP_MAX_OCTAVES)
      throw Error("InvalidData", "normal-perturbation.octaves: 1 to " + std::to_string(RTC_BUMP_MAX_OCTAVES));
    b.octaves = static_cast<uint32_t>(n);
  }
  if (const Value* v = presentField(cfg, "persistence")) {
    if (b.kind != RTC_BUMP_NOISE) throw Error("InvalidData", "normal-perturbation.persistence: of \"noise\" only");
    b.persistence = asFloat(*v, "normal-perturbation.persistence");
    if (!std::isfinite(b.persistence)) throw Error("InvalidData", "normal-perturbation.persistence: a finite number");
  }
  if (const Value* v = presentField(cfg, "transform")) {
    const Matrix4 m = parseTransform(*v);
    try {
      b.inverse = m.inverse();
    } catch (const Error&) {  // (NotInvertible, named by its key here)
      throw Error("InvalidData", "normal-perturbation.transform: an invertible transform");
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 4; ++c)
        if (!std::isfinite(b.inverse.d[r][c])) throw Error("InvalidData", "normal-perturbation.transform: an invertible transform");
  }
  return b;
}

// A material's "roughness" (not in the reference): a number, meaning both values, or
// {"reflection": a, "transmission": b} (either may be absent: 0); each finite and in [0, 1].
Roughness parseRoughness(const Value& cfg) {
  auto one = [](const Value& v, const char* key) {
    if (v.type != Value::Number) throw Error("InvalidData", std::string(key) + ": a number in [0, 1]");
    const double x = asFloat(v, key);
    if (!(std::isfinite(x) && x >= 0.0 && x <= 1.0)) throw Error("InvalidData", std::string(key) + ": a number in [0, 1]");
    return x;
  };
  Roughness r;
  r.present = true;
  if (cfg.type == Value::Object) {
    checkFields(cfg, {"reflection", "transmission"}, "roughness");
    if (const Value* v = presentField(cfg, "reflection")) r.reflection = one(*v, "roughness.reflection");
    if (const Value* v = presentField(cfg, "transmission")) r.transmission = one(*v, "roughness.transmission");
  } else {
    r.reflection = r.transmission = one(cfg, "roughness");
  }
  return r;
}

// A material's "ambient-occlusion" (not in the reference): a number, the radius, or {"radius": r}
// (absent: 0); finite and >= 0.
Occlusion parseOcclusion(const Value& cfg) {
  auto one = [](const Value& v, const char* key) {
    if (v.type != Value::Number) throw Error("InvalidData", std::string(key) + ": a number >= 0");
    const double x = asFloat(v, key);
    if (!(std::isfinite(x) && x >= 0.0)) throw Error("InvalidData", std::string(key) + ": a number >= 0");
    return x;
  };
  Occlusion o;
  o.present = true;
  if (cfg.type == Value::Object) {
    checkFields(cfg, {"radius"}, "ambient-occlusion");
    if (const Value* v = presentField(cfg, "radius")) o.radius = one(*v, "ambient-occlusion.radius");
  } else {
    o.radius = one(cfg, "ambient-occlusion");
  }
  return o;
}

// A material's "shadow-filter" (not in the reference): a number f - (f, f, f) -, [r, g, b], or true
// - the material's transparency in each channel, taken by parseMaterial once the material's own keys are read -; each
// value finite and in [0, 1].
ShadowFilter parseShadowFilter(const Value& cfg) {
  auto one = [](const Value& v) {
    if (v.type != Value::Number) throw Error("InvalidData", "shadow-filter: a number in [0, 1], [r, g, b] or true");
    const double x = asFloat(v, "shadow-filter");
    if (!(std::isfinite(x) && x >= 0.0 && x <= 1.0)) throw Error("InvalidData", "shadow-filter: a number in [0, 1]");
    return x;
  };
  ShadowFilter f;
  f.present = true;
  if (cfg.type == Value::Bool) {
    if (!cfg.b) throw Error("InvalidData", "shadow-filter: a number in [0, 1], [r, g, b] or true");
    f.from_transparency = true;
  } else if (cfg.type == Value::Array) {
    if (cfg.arr.size() != 3) throw Error("LengthMismatch", "shadow-filter: [r, g, b]");
    f.r = one(cfg.arr[0]);
    f.g = one(cfg.arr[1]);
    f.b = one(cfg.arr[2]);
  } else {
    f.r = f.g = f.b = one(cfg);
  }
  return f;
}

// A material's "absorption" (not in the reference): a number a - (a, a, a) -, [r, g, b], or
// {"color": [r, g, b], "distance": d} - white light has that colour after d units inside the material: -log(color.c) / d,
// color.c in (0, 1], d > 0 and finite; a -0.0 is stored as 0.0 -; each value finite and >= 0.
Absorption parseAbsorption(const Value& cfg) {
  auto one = [](const Value& v) {
    if (v.type != Value::Number) throw Error("InvalidData", "absorption: a number >= 0, [r, g, b] or {color, distance}");
    const double x = asFloat(v, "absorption");
    if (!(std::isfinite(x) && x >= 0.0)) throw Error("InvalidData", "absorption: a finite number >= 0");
    return x;
  };
  Absorption a;
  a.present = true;
  if (cfg.type == Value::Object) {
    checkFields(cfg, {"color", "distance"}, "absorption");
    const Value& col = requireField(cfg, "color", "absorption");
    if (col.type != Value::Array) throw Error("InvalidData", "absorption: color is [r, g, b]");
    if (col.arr.size() != 3) throw Error("LengthMismatch", "absorption: color is [r, g, b]");
    const Value& dv = requireField(cfg, "distance", "absorption");
    if (dv.type != Value::Number) throw Error("InvalidData", "absorption: distance is a number > 0");
    const double d = asFloat(dv, "absorption");
    if (!(std::isfinite(d) && d > 0.0)) throw Error("InvalidData", "absorption: distance is a finite number > 0");
    double s[3];
    for (int i = 0; i < 3; ++i) {
      if (col.arr[i].type != Value::Number) throw Error("InvalidData", "absorption: color is three numbers in (0, 1]");
      const double c = asFloat(col.arr[i], "absorption");
      if (!(c > 0.0 && c <= 1.0)) throw Error("InvalidData", "absorption: color is three numbers in (0, 1]");
      const double v = -std::log(c) / d;
      if (!std::isfinite(v)) throw Error("InvalidData", "absorption: color and distance give a value that is not finite");
      s[i] = v == 0.0 ? 0.0 : v;  // (-0.0 is stored as 0.0)
    }
    a.r = s[0];
    a.g = s[1];
    a.b = s[2];
  } else if (cfg.type == Value::Array) {
    if (cfg.arr.size() != 3) throw Error("LengthMismatch", "absorption: [r, g, b]");
    a.r = one(cfg.arr[0]);
    a.g = one(cfg.arr[1]);
    a.b = one(cfg.arr[2]);
  } else {
    a.r = a.g = a.b = one(cfg);
  }
  return a;
}

// A material's "emission" (not in the reference): a number e - (e, e, e) - or [r, g, b]; each value
// finite and >= 0.
Emission parseEmission(const Value& cfg) {
  auto one = [](const Value& v) {
    if (v.type != Value::Number) throw Error("InvalidData", "emission: a number >= 0 or [r, g, b]");
    const double x = asFloat(v, "emission");
    if (!(std::isfinite(x) && x >= 0.0)) throw Error("InvalidData", "emission: a finite number >= 0");
    return x == 0.0 ? 0.0 : x;  // (-0.0 is stored as 0.0)
  };
  Emission e;
  e.present = true;
  if (cfg.type == Value::Array) {
    if (cfg.arr.size() != 3) throw Error("LengthMismatch", "emission: [r, g, b]");
    e.r = one(cfg.arr[0]);
    e.g = one(cfg.arr[1]);
    e.b = one(cfg.arr[2]);
  } else {
    e.r = e.g = e.b = one(cfg);
  }
  return e;
}

Material parseMaterial(const Value& cfg, const std::optional<Material>& inherited, const FileLoader& load_file_data) {
  requireObject(cfg, "material");
  checkFields(cfg, {"pattern", "ambient", "diffuse", "specular", "shininess", "reflective", "transparency",
                    "refractive-index", "normal-perturbation", "roughness", "ambient-occlusion", "shadow-filter", "absorption", "emission"}, "material");
  Material mat = inherited ? *inherited : Material{};
  auto present = [&](const char* k) -> const Value* {
    const Value* v = cfg.find(k);
    return (v && v->type != Value::Null) ? v : nullptr;
  };
  if (auto* v = present("pattern")) mat.pattern = parsePattern(*v, load_file_data);
  if (auto* v = present("ambient")) mat.ambient = asFloat(*v, "ambient");
  if (auto* v = present("diffuse")) mat.diffuse = asFloat(*v, "diffuse");
  if (auto* v = present("specular")) mat.specular = asFloat(*v, "specular");
  if (auto* v = present("shininess")) mat.shininess = asFloat(*v, "shininess");
  if (auto* v = present("reflective")) mat.reflective = asFloat(*v, "reflective");
  if (auto* v = present("transparency")) mat.transparency = asFloat(*v, "transparency");
  if (auto* v = present("refractive-index")) mat.refractive_index = asFloat(*v, "refractive-index");
  if (auto* v = present("normal-perturbation")) mat.bump = parseBump(*v);
  if (auto* v = present("roughness")) mat.roughness = parseRoughness(*v);
  if (auto* v = present("ambient-occlusion")) mat.occlusion = parseOcclusion(*v);
  if (auto* v = present("shadow-filter")) mat.shadow_filter = parseShadowFilter(*v);
  if (auto* v = present("absorption")) mat.absorption = parseAbsorption(*v);
  if (auto* v = present("emission")) mat.emission = parseEmission(*v);
  if (mat.shadow_filter.from_transparency) {  // (`true`, the material's own or an inherited one: this material's transparency)
    const double t = mat.transparency;
    if (!(std::isfinite(t) && t >= 0.0 && t <= 1.0)) throw Error("InvalidData", "shadow-filter: true needs a transparency in [0, 1]");
    mat.shadow_filter.r = mat.shadow_filter.g = mat.shadow_filter.b = t;
  }
  return mat;
}

struct InheritedState {  // scene.zig:432-438
  std::optional<Material> material;
  Matrix4 transform = Matrix4::identity();
  std::optional<bool> casts_shadow;
};

struct Info {
  std::optional<Material> material;
  Matrix4 transform;
  std::optional<bool> casts_shadow;
};

// scene.zig:164-190
Info inherit(const Value& object, const InheritedState& inherited, const FileLoader& load_file_data) {
  Info info;
  if (const Value* m = presentField(object, "material")) {
    info.material = parseMaterial(*m, inherited.material, load_file_data);
  } else {
    info.material = inherited.material;
  }
  if (const Value* t = presentField(object, "transform")) {
    info.transform = parseTransform(*t).mul(inherited.transform);
  } else {
    info.transform = inherited.transform;
  }
  if (const Value* s = presentField(object, "casts-shadow")) {
    info.casts_shadow = asBool(*s, "casts-shadow");
  } else {
    info.casts_shadow = inherited.casts_shadow;
  }
  return info;
}

using Definitions = std::map<std::string, const Value*>;

void parseMinMaxClosed(const Value& cfg, const char* what, Shape& s) {  // scene.zig:134-143
  requireObject(cfg, what);
  checkFields(cfg, {"min", "max", "closed"}, what);
  if (auto* v = cfg.find("min")) s.ymin = asFloat(*v, "min");
  if (auto* v = cfg.find("max")) s.ymax = asFloat(*v, "max");
  if (auto* v = cfg.find("closed")) s.closed = asBool(*v, "closed");
}

// scene.zig:440-591
Shape parseObject(const Value& object, const InheritedState& inherited, const Definitions& definitions,
                  const FileLoader& load_file_data, int depth = 0) {
  if (depth > 64) throw Error("StackOverflow", "shape definitions nest too deeply (cycle?)");
  requireObject(object, "object");
  checkFields(object, {"type", "transform", "material", "casts-shadow", "motion"}, "object");
  // (motion blur, DESIGN.md section 14: only a World.objects entry moves - parseScene reads its "motion" -, not a group's
  // child, a csg operand or a shape definition's body)
  if (depth != 0 && object.find("motion"))
    throw Error("InvalidData", "object: \"motion\" is allowed on a top-level object only (not inside a group, a csg or a definition)");

  const Info info = inherit(object, inherited, load_file_data);
  std::optional<Material> material = info.material;
  Matrix4 transform = info.transform;
  std::optional<bool> casts_shadow = info.casts_shadow;

  const auto& kv = unionMember(requireField(object, "type", "object"), "object.type");
  const std::string& t = kv.first;
  const Value& payload = kv.second;

  Shape shape;
  if (t == "from-definition") {
    const std::string& name = asString(payload, "from-definition");
    auto it = definitions.find(name);
    if (it == definitions.end()) throw Error("UnknownDefinition", name);
    // scene.zig:455-492: the definition is parsed with THIS object's merged material and
    // shadow flag but only the inherited transform; then this object's own fields are
    // inherited again on top of what the parsed definition ended up with.
    InheritedState for_def;
    for_def.material = material;
    for_def.transform = inherited.transform;
    for_def.casts_shadow = casts_shadow;
    Shape parent = parseObject(*it->second, for_def, definitions, load_file_data, depth + 1);
    InheritedState parent_state;
    parent_state.material = parent.material;
    parent_state.transform = parent.transform;
    parent_state.casts_shadow = parent.casts_shadow;
    const Info again = inherit(object, parent_state, load_file_data);
    material = again.material;
    transform = again.transform;
    casts_shadow = again.casts_shadow;
    shape = std::move(parent);
  } else if (t == "from-obj") {
    const Value& cfg = requireObject(payload, "from-obj");
    checkFields(cfg, {"file", "normalize", "texture-coordinates"}, "from-obj");
    const std::string& file = asString(requireField(cfg, "file", "from-obj"), "file");
    bool normalize = true;  // scene.zig:124-127
    if (auto* v = cfg.find("normalize")) normalize = asBool(*v, "normalize");
    const std::string obj = load_file_data(file);
    ObjParser parser;
    if (auto* v = cfg.find("texture-coordinates")) parser.texture_coordinates = asBool(*v, "texture-coordinates");  // 
    ObjParser::InheritedState st;
    st.material = material;
    st.casts_shadow = casts_shadow;
    parser.loadObj(obj, st, normalize);
    shape = parser.takeGroup();
  } else if (t == "sphere") {
    requireVoid(payload, "sphere");
    shape = Shape::sphere();
  } else if (t == "plane") {
    requireVoid(payload, "plane");
    shape = Shape::plane();
  } else if (t == "cube") {
    requireVoid(payload, "cube");
    shape = Shape::cube();
  } else if (t == "cylinder") {
    shape = Shape::cylinder();
    parseMinMaxClosed(payload, "cylinder", shape);
  } else if (t == "cone") {
    shape = Shape::cone();
    parseMinMaxClosed(payload, "cone", shape);
  } else if (t == "torus") {  // (not in the reference): {"major-radius": R, "minor-radius": r}, a ring torus
    const Value& cfg = requireObject(payload, "torus");
    checkFields(cfg, {"major-radius", "minor-radius"}, "torus");
    double major = 1.0, minor = 0.25;
    if (auto* v = cfg.find("major-radius")) major = asFloat(*v, "torus.major-radius");
    if (auto* v = cfg.find("minor-radius")) minor = asFloat(*v, "torus.minor-radius");
    if (!std::isfinite(major)) throw Error("InvalidData", "torus.major-radius: not finite");
    if (!std::isfinite(minor)) throw Error("InvalidData", "torus.minor-radius: not finite");
    if (!(minor > 0.0)) throw Error("InvalidData", "torus.minor-radius: must be above 0");
    if (!(minor < major)) throw Error("InvalidData", "torus.minor-radius: must be below torus.major-radius (a ring torus)");
    shape = Shape::torus(major, minor);
  } else if (t == "triangle") {
    const Value& cfg = requireObject(payload, "triangle");
    checkFields(cfg, {"p1", "p2", "p3", "uv1", "uv2", "uv3"}, "triangle");
    double a[3], b[3], c[3];
    asVec3(requireField(cfg, "p1", "triangle"), "p1", a);
    asVec3(requireField(cfg, "p2", "triangle"), "p2", b);
    asVec3(requireField(cfg, "p3", "triangle"), "p3", c);
    shape = Shape::triangle(Tuple::point(a[0], a[1], a[2]), Tuple::point(b[0], b[1], b[2]),
                            Tuple::point(c[0], c[1], c[2]));
    // (not in the reference) "uv1", "uv2", "uv3": [u, v] of p1, p2, p3 - together or not at all
    const char* const uv_keys[3] = {"uv1", "uv2", "uv3"};
    const bool any_uv = cfg.find("uv1") || cfg.find("uv2") || cfg.find("uv3");
    for (int k = 0; k < 3 && any_uv; ++k) {
      const Value* v = cfg.find(uv_keys[k]);
      if (!v) throw Error("MissingField", std::string("triangle.") + uv_keys[k] + ": uv1, uv2 and uv3 go together");
      if (v->type != Value::Array || v->arr.size() != 2)
        throw Error("InvalidData", std::string("triangle.") + uv_keys[k] + ": expected [u, v]");
      for (int j = 0; j < 2; ++j) {
        const double x = asFloat(v->arr[j], (std::string("triangle.") + uv_keys[k]).c_str());
        if (!std::isfinite(x)) throw Error("InvalidData", std::string("triangle.") + uv_keys[k] + ": not finite");
        shape.tex_uv[2 * k + j] = x;
      }
    }
  } else if (t == "group") {
    requireArray(payload, "group");
    shape = Shape::group();
    for (const Value& child : payload.arr) {
      // Groups push their own transform down in setTransform; children are parsed with
      // the inherited material / shadow flag but an identity transform (scene.zig:527-546).
      InheritedState st;
      st.material = material;
      st.casts_shadow = casts_shadow;
      shape.addChild(parseObject(child, st, definitions, load_file_data, depth + 1));
    }
  } else if (t == "csg") {  // scene.zig:547-575
    requireObject(payload, "csg");
    checkFields(payload, {"left", "right", "operation"}, "csg");
    InheritedState st;
    st.material = material;
    st.casts_shadow = casts_shadow;
    Shape left = parseObject(requireField(payload, "left", "csg"), st, definitions, load_file_data, depth + 1);
    Shape right = parseObject(requireField(payload, "right", "csg"), st, definitions, load_file_data, depth + 1);
    const std::string& op = asString(requireField(payload, "operation", "csg"), "operation");
    CsgOp o;
    if (op == "union") {
      o = CsgOp::Union;
    } else if (op == "intersection") {
      o = CsgOp::Intersection;
    } else if (op == "difference") {
      o = CsgOp::Difference;
    } else {
      throw Error("InvalidEnumTag", "csg.operation " + op);
    }
    shape = Shape::csg(std::move(left), std::move(right), o);
  } else {
    throw Error("UnknownField", "object.type." + t);
  }

  shape.setTransform(transform);           // scene.zig:578
  if (material) shape.material = *material;  // scene.zig:580-582
  if (casts_shadow) shape.casts_shadow = *casts_shadow;
  shape.divide(8);                         // scene.zig:588
  return shape;
}

}  // namespace

namespace {
std::atomic<unsigned> g_loader_threads{0};
}
void setLoaderThreads(unsigned threads) { g_loader_threads.store(threads); }
unsigned loaderThreads() {
  const unsigned asked = g_loader_threads.load();
  if (asked) return asked;
  unsigned n = std::max(1u, std::thread::hardware_concurrency());
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = std::min<unsigned>(n, std::max(1, CPU_COUNT(&set)));
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "<quota> <period>" or "max <period>"
    long long quota = 0, period = 0;
    if (std::fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0)
      n = std::min<unsigned>(n, static_cast<unsigned>(std::max<long long>(1, quota / period)));
    std::fclose(f);
  }
  return std::min(16u, n);
}

// ---- scene.zig:612-661 ------------------------------------------------------------------
SceneInfo parseScene(const std::string& scene_json, const FileLoader& load_file_data) {
  const Value root = json::parse(scene_json);
  requireObject(root, "scene");
  checkFields(root, {"shape-definitions", "camera", "lights", "objects", "atmosphere", "environment", "indirect"}, "scene");

  Definitions definitions;
  if (const Value* defs = root.find("shape-definitions")) {
    requireArray(*defs, "shape-definitions");
    for (const Value& d : defs->arr) {
      requireObject(d, "shape-definition");
      checkFields(d, {"name", "value"}, "shape-definition");
      const std::string& name = asString(requireField(d, "name", "shape-definition"), "name");
      definitions[name] = &requireField(d, "value", "shape-definition");  // put(): last one wins
    }
  }

  const Value& cam = requireObject(requireField(root, "camera", "scene"), "camera");
  checkFields(cam, {"width", "height", "field-of-view", "from", "to", "up", "sampling", "film"}, "camera");
  SceneInfo info;
  info.camera = Camera::create(asUsize(requireField(cam, "width", "camera"), "width"),
                               asUsize(requireField(cam, "height", "camera"), "height"),
                               asFloat(requireField(cam, "field-of-view", "camera"), "field-of-view"));
  double f[3], t[3], u[3];
  asVec3(requireField(cam, "from", "camera"), "from", f);
  asVec3(requireField(cam, "to", "camera"), "to", t);
  asVec3(requireField(cam, "up", "camera"), "up", u);
  const Tuple from = Tuple::point(f[0], f[1], f[2]);
  const Tuple to = Tuple::point(t[0], t[1], t[2]);
  const Tuple up = Tuple::vec3(u[0], u[1], u[2]);
  // "atmosphere" (not in the reference): the uniform fog outside every solid
  if (const Value* atm = root.find("atmosphere")) {
    requireObject(*atm, "atmosphere");
    checkFields(*atm, {"density", "color"}, "atmosphere");
    info.atmosphere_present = true;
    const Value& dv = requireField(*atm, "density", "atmosphere");
    if (dv.type != Value::Number) throw Error("InvalidData", "atmosphere: density is a number >= 0");
    info.fog_density = asFloat(dv, "atmosphere");
    if (!(std::isfinite(info.fog_density) && info.fog_density >= 0.0)) throw Error("InvalidData", "atmosphere: density is a finite number >= 0");
    const Value& col = requireField(*atm, "color", "atmosphere");
    if (col.type != Value::Array) throw Error("InvalidData", "atmosphere: color is [r, g, b]");
    if (col.arr.size() != 3) throw Error("LengthMismatch", "atmosphere: color is [r, g, b]");
    for (int i = 0; i < 3; ++i) {
      if (col.arr[i].type != Value::Number) throw Error("InvalidData", "atmosphere: color is three numbers >= 0");
      info.fog_color[i] = asFloat(col.arr[i], "atmosphere");
      if (!(std::isfinite(info.fog_color[i]) && info.fog_color[i] >= 0.0)) throw Error("InvalidData", "atmosphere: color is three finite numbers >= 0");
    }
  }
  // "environment" (not in the reference): the sky behind the world and the suns that light it
  if (const Value* env = root.find("environment")) {
    requireObject(*env, "environment");
    checkFields(*env, {"color", "pattern", "projection", "suns", "light"}, "environment");
    if (env->obj.empty()) throw Error("MissingField", "environment: one of color, pattern, projection, suns, light");
    info.environment_present = true;
    // (three finite numbers >= 0)
    auto vec3 = [](const Value& v, const char* what, double out[3]) {
      if (v.type != Value::Array) throw Error("InvalidData", std::string(what) + " is [x, y, z]");
      if (v.arr.size() != 3) throw Error("LengthMismatch", std::string(what) + " is [x, y, z]");
      for (int i = 0; i < 3; ++i) {
        if (v.arr[i].type != Value::Number) throw Error("InvalidData", std::string(what) + " is three numbers");
        out[i] = v.arr[i].num;
        if (!std::isfinite(out[i])) throw Error("InvalidData", std::string(what) + " is three finite numbers");
      }
    };
    auto colour = [&](const Value& v, const char* what, double out[3]) {
      vec3(v, what, out);
      for (int i = 0; i < 3; ++i)
        if (!(out[i] >= 0.0)) throw Error("InvalidData", std::string(what) + " is three numbers >= 0");
    };
    if (const Value* p = env->find("pattern")) {
      info.env_pattern = parsePattern(*p, load_file_data);
      if (hasMeshMap(*info.env_pattern)) throw Error("InvalidData", "environment: a mesh texture map has no triangle to read");
      info.env_color[0] = info.env_color[1] = info.env_color[2] = 1.0;
    }
    if (const Value* c = env->find("color")) colour(*c, "environment: color", info.env_color);
    if (const Value* pr = env->find("projection")) {
      if (pr->type != Value::String) throw Error("InvalidData", "environment: projection is \"sphere\" or \"cube\"");
      if (pr->str == "cube") {
        info.env_projection = RTC_ENV_CUBE;
      } else if (pr->str != "sphere") {
        throw Error("InvalidData", "environment: projection is \"sphere\" or \"cube\"");
      }
    }
    if (const Value* suns = env->find("suns")) {
      if (suns->type != Value::Array) throw Error("InvalidData", "environment: suns is a list");
      if (suns->arr.size() > RTC_ENV_MAX_SUNS) throw Error("InvalidData", "environment: more than " + std::to_string(RTC_ENV_MAX_SUNS) + " suns");
      for (const Value& sun : suns->arr) {
        requireObject(sun, "sun");
        checkFields(sun, {"direction", "intensity"}, "sun");
        double d[3], c[3];
        vec3(requireField(sun, "direction", "sun"), "sun: direction", d);
        colour(requireField(sun, "intensity", "sun"), "sun: intensity", c);
        const double len = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        if (!(std::isfinite(len) && len > 0.0)) throw Error("InvalidData", "sun: a direction of zero or non-finite magnitude");
        info.sun_direction.insert(info.sun_direction.end(), d, d + 3);
        info.sun_intensity.insert(info.sun_intensity.end(), c, c + 3);
      }
    }
    // "light" (DESIGN.md section 25): the sky lights diffuse surfaces - a gain, or {"gain", "samples", "seed"}; no table row
    if (const Value* light = env->find("light")) {
      auto gainOf = [](const Value& v) {
        if (v.type != Value::Number) throw Error("InvalidData", "environment: light: gain is a number");
        if (!(std::isfinite(v.num) && v.num >= 0.0)) throw Error("InvalidData", "environment: light: gain is a finite number >= 0");
        return v.num;
      };
      // (a whole number in [lo, hi])
      auto wholeOf = [](const Value& v, const std::string& what, double lo, double hi) {
        if (v.type != Value::Number || !(v.num >= lo && v.num <= hi) || v.num != std::floor(v.num))
          throw Error("InvalidData", std::string("environment: light: ") + what);
        return v.num;
      };
      info.sky_light_present = true;
      info.sky_light_gain = 1.0;
      if (light->type == Value::Object) {
        checkFields(*light, {"gain", "samples", "seed"}, "light");
        if (const Value* g = light->find("gain")) info.sky_light_gain = gainOf(*g);
        if (const Value* n = light->find("samples"))
          info.sky_light_samples = static_cast<uint32_t>(wholeOf(*n, "samples is a whole number from 1 to " + std::to_string(RTC_SKY_LIGHT_MAX_SAMPLES), 1.0, RTC_SKY_LIGHT_MAX_SAMPLES));
        if (const Value* sd = light->find("seed")) info.sky_light_seed = static_cast<uint64_t>(wholeOf(*sd, "seed is a whole number from 0 to 2^53", 0.0, 0x1p53));
      } else {
        info.sky_light_gain = gainOf(*light);
      }
      const bool has_sky = info.env_pattern.has_value() || info.env_color[0] != 0.0 || info.env_color[1] != 0.0 || info.env_color[2] != 0.0;
      if (!has_sky) throw Error("InvalidData", "environment: light in an environment that has no sky (no pattern and a colour of zero)");
    }
  }
  // "indirect" (not in the reference): diffuse bounce rays - a gain, or {"gain", "bounces", "seed"};
  // no table row
  if (const Value* ind = root.find("indirect")) {
    auto gainOf = [](const Value& v) {
      if (v.type != Value::Number) throw Error("InvalidData", "indirect: gain is a number");
      if (!(std::isfinite(v.num) && v.num >= 0.0)) throw Error("InvalidData", "indirect: gain is a finite number >= 0");
      return v.num;
    };
    // (a whole number in [lo, hi])
    auto wholeOf = [](const Value& v, const std::string& what, double lo, double hi) {
      if (v.type != Value::Number || !(v.num >= lo && v.num <= hi) || v.num != std::floor(v.num))
        throw Error("InvalidData", std::string("indirect: ") + what);
      return v.num;
    };
    info.indirect_present = true;
    info.indirect_gain = 1.0;
    info.indirect_bounces = 1u;
    if (ind->type == Value::Object) {
      checkFields(*ind, {"gain", "bounces", "seed", "emitters"}, "indirect");
      if (const Value* g = ind->find("gain")) info.indirect_gain = gainOf(*g);
      if (const Value* n = ind->find("bounces")) info.indirect_bounces = static_cast<uint32_t>(wholeOf(*n, "bounces is a whole number from 0 to 16", 0.0, 16.0));
      if (const Value* sd = ind->find("seed")) info.indirect_seed = static_cast<uint64_t>(wholeOf(*sd, "seed is a whole number from 0 to 2^53", 0.0, 0x1p53));
      // "emitters" (DESIGN.md section 28): emissive surfaces sampled directly - true, a sample count, or {"samples", "seed"};
      // false: no table, as without the key
      if (const Value* em = ind->find("emitters")) {
        const char* const samples_are = "emitters: samples is a whole number from 1 to 16";
        if (em->type == Value::Bool) {
          info.emitters_present = em->b;
        } else if (em->type == Value::Number) {
          info.emitters_present = true;
          info.emitters_samples = static_cast<uint32_t>(wholeOf(*em, samples_are, 1.0, 16.0));
        } else if (em->type == Value::Object) {
          checkFields(*em, {"samples", "seed", "mis"}, "emitters");
          info.emitters_present = true;
          // "mis" (DESIGN.md section 32): the samples and the diffuse child weighted by the balance heuristic; false: as
          // without the key
          if (const Value* mi = em->find("mis")) {
            if (mi->type != Value::Bool) throw Error("InvalidData", "emitters: mis is true or false");
            info.emitters_mis = mi->b;
          }
          if (const Value* n = em->find("samples")) info.emitters_samples = static_cast<uint32_t>(wholeOf(*n, samples_are, 1.0, 16.0));
          if (const Value* sd = em->find("seed"))
            info.emitters_seed = static_cast<uint64_t>(wholeOf(*sd, "emitters: seed is a whole number from 0 to 2^53", 0.0, 0x1p53));
        } else {
          throw Error("InvalidData", "indirect: emitters is true, a sample count or {\"samples\", \"seed\", \"mis\"}");
        }
      }
    } else {
      info.indirect_gain = gainOf(*ind);
    }
  }
  info.camera.saved_from = from;
  info.camera.saved_to = to;
  info.camera.saved_up = up;
  info.camera.setTransform(Matrix4::viewTransform(from, to, up));
  if (const Value* smp = cam.find("sampling")) {  // (not in the reference: anti-aliasing and focal blur, every key optional)
    requireObject(*smp, "sampling");
    checkFields(*smp, {"grid", "jitter", "aperture", "focal-distance", "seed", "passes", "adaptive", "denoise", "robust", "gloss-seed",
                       "occlusion-samples", "occlusion-seed"}, "sampling");
    CameraSampling& s = info.sampling;
    if (const Value* v = smp->find("grid")) {
      const size_t g = asUsize(*v, "grid");
      if (g < 1 || g > 16) throw Error("InvalidData", "sampling: grid is 1 to 16");
      s.grid = static_cast<uint32_t>(g);
    }
    if (const Value* v = smp->find("jitter")) s.jitter = asBool(*v, "jitter");
    if (const Value* v = smp->find("aperture")) s.aperture = asFloat(*v, "aperture");
    if (!std::isfinite(s.aperture) || s.aperture < 0.0) throw Error("InvalidData", "sampling: aperture is finite and at least 0");
    if (const Value* v = smp->find("focal-distance")) {
      s.focal_distance = asFloat(*v, "focal-distance");
      if (!std::isfinite(s.focal_distance) || s.focal_distance <= 0.0) throw Error("InvalidData", "sampling: focal-distance is finite and above 0");
    } else if (s.aperture > 0.0) {  // focused on the point the camera looks at
      const double dx = t[0] - f[0], dy = t[1] - f[1], dz = t[2] - f[2];
      s.focal_distance = std::sqrt((dx * dx + dy * dy) + dz * dz);
      if (!(s.focal_distance > 0.0)) throw Error("InvalidData", "sampling: from == to, and no focal-distance");
    }
    if (const Value* v = smp->find("seed")) s.seed = static_cast<uint64_t>(asUsize(*v, "seed"));
    if (const Value* v = smp->find("gloss-seed")) s.gloss_seed = static_cast<uint64_t>(asUsize(*v, "gloss-seed"));  // (section 20)
    if (const Value* v = smp->find("occlusion-samples")) {  // (section 21)
      const size_t n = asUsize(*v, "occlusion-samples");
      if (n < 1 || n > RTC_OCCLUSION_MAX_SAMPLES) throw Error("InvalidData", "occlusion-samples: 1 .. " + std::to_string(RTC_OCCLUSION_MAX_SAMPLES));
      s.occlusion_samples = static_cast<uint32_t>(n);
    }
    if (const Value* v = smp->find("occlusion-seed")) s.occlusion_seed = static_cast<uint64_t>(asUsize(*v, "occlusion-seed"));
    if (const Value* v = smp->find("passes")) {  // (progressive rendering, DESIGN.md section 13: sample passes 0 .. passes-1)
      const size_t n = asUsize(*v, "passes");
      const size_t most = RTC_SAMPLING_INDEX_LIMIT / (static_cast<size_t>(s.grid) * s.grid);
      if (n < 1 || n > most) throw Error("InvalidData", "sampling: passes is 1 to " + std::to_string(most) + " at grid " + std::to_string(s.grid));
      s.passes = static_cast<uint32_t>(n);
    }
    if (const Value* ad = smp->find("adaptive")) {  // (adaptive sampling, DESIGN.md section 15: "passes" is the maximum)
      requireObject(*ad, "adaptive");
      checkFields(*ad, {"threshold", "min-passes", "tile"}, "sampling.adaptive");
      s.adaptive = true;
      s.threshold = asFloat(requireField(*ad, "threshold", "sampling.adaptive"), "threshold");
      if (!std::isfinite(s.threshold) || s.threshold < 0.0) throw Error("InvalidData", "sampling.adaptive: threshold is finite and at least 0");
      if (const Value* v = ad->find("min-passes")) {
        const size_t n = asUsize(*v, "min-passes");
        if (n < 2 || n > s.passes)
          throw Error("InvalidData", "sampling.adaptive: min-passes is 2 to passes (" + std::to_string(s.passes) + ")");
        s.min_passes = static_cast<uint32_t>(n);
      }
      if (s.passes < s.min_passes)
        throw Error("InvalidData", "sampling.adaptive: passes (" + std::to_string(s.passes) + ") is below min-passes (" +
                                       std::to_string(s.min_passes) + ")");
      if (const Value* v = ad->find("tile")) {
        size_t wh[2];
        if (v->type == Value::Array) {
          if (v->arr.size() != 2) throw Error("LengthMismatch", "tile");
          for (int i = 0; i < 2; ++i) wh[i] = asUsize(v->arr[i], "tile");
        } else {
          wh[0] = wh[1] = asUsize(*v, "tile");
        }
        for (size_t d : wh)
          if (d < 1 || d > RTC_ADAPTIVE_MAX_TILE) throw Error("InvalidData", "sampling.adaptive: tile is 1 to " + std::to_string(RTC_ADAPTIVE_MAX_TILE));
        s.tile_w = static_cast<uint32_t>(wh[0]);
        s.tile_h = static_cast<uint32_t>(wh[1]);
      }
    }
    if (const Value* dn = smp->find("denoise")) {  // (the denoiser, DESIGN.md section 29: true, false or the setting's keys)
      if (dn->type == Value::Object) {
        checkFields(*dn, {"radius", "patch", "strength", "cancel"}, "sampling.denoise");
        s.denoise = true;
        auto wholeOf = [](const Value& v, const std::string& what, double hi) {
          if (v.type != Value::Number || !(v.num >= 0.0 && v.num <= hi) || v.num != std::floor(v.num))
            throw Error("InvalidData", "sampling.denoise: " + what + " is a whole number from 0 to " + std::to_string(static_cast<unsigned>(hi)));
          return static_cast<uint32_t>(v.num);
        };
        auto realOf = [](const Value& v, const std::string& what, bool zero) {
          if (v.type != Value::Number || !std::isfinite(v.num) || v.num < 0.0 || (!zero && v.num == 0.0))
            throw Error("InvalidData", "sampling.denoise: " + what + (zero ? " is finite and at least 0" : " is finite and above 0"));
          return v.num;
        };
        if (const Value* v = dn->find("radius")) s.denoise_radius = wholeOf(*v, "radius", RTC_DENOISE_MAX_RADIUS);
        if (const Value* v = dn->find("patch")) s.denoise_patch = wholeOf(*v, "patch", RTC_DENOISE_MAX_PATCH);
        if (const Value* v = dn->find("strength")) s.denoise_strength = realOf(*v, "strength", false);
        if (const Value* v = dn->find("cancel")) s.denoise_cancel = realOf(*v, "cancel", true);
      } else if (dn->type == Value::Bool) {
        s.denoise = dn->b;
      } else {
        throw Error("InvalidData", "sampling: denoise is true, false or {\"radius\", \"patch\", \"strength\", \"cancel\"}");
      }
      if (s.denoise && !s.adaptive && s.passes < 2)
        throw Error("InvalidData", "sampling: denoise needs passes of 2 or more, or adaptive");
    }
    if (const Value* rb = smp->find("robust")) {  // (robust accumulation, DESIGN.md section 31: true, false, M or the setting's keys)
      auto bucketsOf = [](const Value& v) {
        if (v.type != Value::Number || !(v.num >= 3.0 && v.num <= RTC_ROBUST_MAX_BUCKETS) || v.num != std::floor(v.num) ||
            static_cast<uint32_t>(v.num) % 2u == 0u)
          throw Error("InvalidData", "sampling.robust: buckets is an odd whole number from 3 to " + std::to_string(RTC_ROBUST_MAX_BUCKETS));
        return static_cast<uint32_t>(v.num);
      };
      if (rb->type == Value::Object) {
        checkFields(*rb, {"buckets", "gain"}, "sampling.robust");
        s.robust = true;
        if (const Value* v = rb->find("buckets")) s.robust_buckets = bucketsOf(*v);
        if (const Value* v = rb->find("gain")) {
          if (v->type != Value::Number || !std::isfinite(v->num) || v->num < 0.0)
            throw Error("InvalidData", "sampling.robust: gain is finite and at least 0");
          s.robust_gain = v->num;
        }
      } else if (rb->type == Value::Bool) {
        s.robust = rb->b;
      } else if (rb->type == Value::Number) {
        s.robust = true;
        s.robust_buckets = bucketsOf(*rb);
      } else {
        throw Error("InvalidData", "sampling: robust is true, false, a bucket count or {\"buckets\", \"gain\"}");
      }
      if (s.robust && s.adaptive) throw Error("InvalidData", "sampling: robust beside adaptive (buckets per tile are not kept)");
      if (s.robust && s.passes < s.robust_buckets)
        throw Error("InvalidData", "sampling: robust needs passes of its " + std::to_string(s.robust_buckets) + " buckets or more");
    }
  }
  if (const Value* fv = cam.find("film")) {  // (the film stage, DESIGN.md section 30: true, false or the setting's keys)
    CameraFilm& f = info.film;
    auto realOf = [](const Value& v, const std::string& what, bool zero) {
      if (v.type != Value::Number || !std::isfinite(v.num) || v.num < 0.0 || (!zero && v.num == 0.0))
        throw Error("InvalidData", "film: " + what + (zero ? " is finite and at least 0" : " is finite and above 0"));
      return v.num;
    };
    if (fv->type == Value::Object) {
      checkFields(*fv, {"exposure", "auto-exposure", "bloom", "tone-curve", "white", "transfer"}, "film");
      f.enabled = true;
      if (const Value* v = fv->find("exposure")) {
        if (v->type == Value::Object) {
          checkFields(*v, {"stops"}, "film.exposure");
          const Value* stops = v->find("stops");
          if (!stops || stops->type != Value::Number || !std::isfinite(stops->num)) throw Error("InvalidData", "film: exposure is {\"stops\": s}, s finite");
          f.exposure = std::exp2(stops->num);
          if (!std::isfinite(f.exposure) || f.exposure <= 0.0) throw Error("InvalidData", "film: exposure stops out of range");
        } else {
          f.exposure = realOf(*v, "exposure", false);
        }
      }
      if (const Value* v = fv->find("auto-exposure")) {
        if (v->type == Value::Bool) f.auto_key = v->b ? 0.18 : 0.0;
        else f.auto_key = realOf(*v, "auto-exposure", true);
      }
      if (const Value* v = fv->find("bloom")) {
        if (v->type == Value::Object) {
          checkFields(*v, {"radius", "sigma", "threshold", "intensity"}, "film.bloom");
          f.bloom_radius = 12u, f.bloom_threshold = 1.0, f.bloom_intensity = 0.15;
          if (const Value* r = v->find("radius")) {
            if (r->type != Value::Number || !(r->num >= 0.0 && r->num <= RTC_FILM_MAX_RADIUS) || r->num != std::floor(r->num))
              throw Error("InvalidData", "film.bloom: radius is a whole number from 0 to " + std::to_string(RTC_FILM_MAX_RADIUS));
            f.bloom_radius = static_cast<uint32_t>(r->num);
          }
          if (f.bloom_radius > 0u) f.bloom_sigma = f.bloom_radius / 3.0;
          if (const Value* r = v->find("sigma")) f.bloom_sigma = realOf(*r, "bloom sigma", false);
          if (const Value* r = v->find("threshold")) f.bloom_threshold = realOf(*r, "bloom threshold", true);
          if (const Value* r = v->find("intensity")) f.bloom_intensity = realOf(*r, "bloom intensity", true);
        } else if (v->type == Value::Bool) {
          if (v->b) f.bloom_radius = 12u, f.bloom_sigma = 4.0, f.bloom_threshold = 1.0, f.bloom_intensity = 0.15;
        } else {
          throw Error("InvalidData", "film: bloom is true, false or {\"radius\", \"sigma\", \"threshold\", \"intensity\"}");
        }
      }
      if (const Value* v = fv->find("tone-curve")) {
        static const char* const names[] = {"linear", "reinhard", "aces", "hable"};
        uint32_t c = 0;
        while (c < 4u && !(v->type == Value::String && v->str == names[c])) ++c;
        if (c == 4u) throw Error("InvalidData", "film: tone-curve is \"linear\", \"reinhard\", \"aces\" or \"hable\"");
        f.curve = c;
      }
      if (const Value* v = fv->find("white")) f.white = realOf(*v, "white", false);
      if (const Value* v = fv->find("transfer")) {
        if (v->type == Value::String && v->str == "linear") {
          f.transfer = RTC_FILM_TRANSFER_LINEAR;
        } else if (v->type == Value::String && v->str == "srgb") {
          f.transfer = RTC_FILM_TRANSFER_SRGB;
        } else if (v->type == Value::Object) {
          checkFields(*v, {"gamma"}, "film.transfer");
          const Value* g = v->find("gamma");
          if (!g) throw Error("InvalidData", "film: transfer is \"linear\", \"srgb\" or {\"gamma\": g}");
          f.transfer = RTC_FILM_TRANSFER_GAMMA;
          f.gamma = realOf(*g, "gamma", false);
        } else {
          throw Error("InvalidData", "film: transfer is \"linear\", \"srgb\" or {\"gamma\": g}");
        }
      }
    } else if (fv->type == Value::Bool) {
      f.enabled = fv->b;
    } else {
      throw Error("InvalidData", "camera: film is true, false or {\"exposure\", \"auto-exposure\", \"bloom\", \"tone-curve\", \"white\", \"transfer\"}");
    }
  }

  const Value& objects = requireArray(requireField(root, "objects", "scene"), "objects");
  // `lights` has no default in SceneConfig (scene.zig:206): it is required.
  const Value& lights = requireArray(requireField(root, "lights", "scene"), "lights");

  // scene.zig:650-655 is one loop; here the objects are built side by side and numbered afterwards, in their order, with
  // the ids that loop would have drawn (dragons.json: six dragons of 23 490 triangles each, 0.5 s of parsing and dividing)
  const size_t n_objects = objects.arr.size();
  const size_t n_threads = std::min<size_t>(n_objects, loaderThreads());
  if (n_threads <= 1) {
    for (const Value& o : objects.arr)
      info.world.objects.push_back(parseObject(o, InheritedState{}, definitions, load_file_data));
  } else {
    std::vector<Shape> built(n_objects);
    std::vector<size_t> ids_drawn(n_objects, 0);
    std::vector<std::exception_ptr> failed(n_objects);
    std::atomic<size_t> next{0};
    auto work = [&] {
      for (size_t i = next.fetch_add(1); i < n_objects; i = next.fetch_add(1)) {
        ShapeIdScope ids;
        try {
          built[i] = parseObject(objects.arr[i], InheritedState{}, definitions, load_file_data);
        } catch (...) {
          failed[i] = std::current_exception();
        }
        ids_drawn[i] = ids.drawn;
      }
    };
    std::vector<std::thread> pool;
    pool.reserve(n_threads);
    try {
      for (size_t t = 1; t < n_threads; ++t) pool.emplace_back(work);
    } catch (const std::system_error&) {
      // (no more threads to be had: the ones that started and this one share the work)
    }
    work();
    for (std::thread& t : pool) t.join();
    for (size_t i = 0; i < n_objects; ++i) {
      if (failed[i]) std::rethrow_exception(failed[i]);  // (the first object in the file's order that fails, as in the one loop)
      offsetShapeIds(built[i], reserveShapeIds(ids_drawn[i]));
      info.world.objects.push_back(std::move(built[i]));
    }
  }

  // (not in the reference: an entry's optional "motion" [dx, dy, dz], its world-space displacement over the shutter)
  info.motion.assign(3 * n_objects, 0.0);
  for (size_t i = 0; i < n_objects; ++i) {
    if (const Value* m = objects.arr[i].find("motion")) {
      asVec3(*m, "motion", &info.motion[3 * i]);
      for (int k = 0; k < 3; ++k)
        if (!std::isfinite(info.motion[3 * i + k])) throw Error("InvalidData", "motion: every component is finite");
    }
  }

  for (const Value& l : lights.arr) {  // scene.zig:593-606
    const auto& kv = unionMember(l, "light");
    if (kv.first == "area-light") {  // the book's bonus chapter: area_light(corner, uvec, usteps, vvec, vsteps, intensity, jitter)
      const Value& cfg = requireObject(kv.second, "area-light");
      checkFields(cfg, {"corner", "uvec", "usteps", "vvec", "vsteps", "intensity", "jitter"}, "area-light");
      double corner[3], u[3], v[3], c[3];
      asVec3(requireField(cfg, "corner", "area-light"), "corner", corner);
      asVec3(requireField(cfg, "uvec", "area-light"), "uvec", u);
      asVec3(requireField(cfg, "vvec", "area-light"), "vvec", v);
      asVec3(requireField(cfg, "intensity", "area-light"), "intensity", c);
      const size_t us = asUsize(requireField(cfg, "usteps", "area-light"), "usteps");
      const size_t vs = asUsize(requireField(cfg, "vsteps", "area-light"), "vsteps");
      if (us == 0 || vs == 0) throw Error("InvalidData", "area-light: usteps and vsteps are at least 1");
      if (us > RTC_AREA_MAX_SAMPLES || vs > RTC_AREA_MAX_SAMPLES || us * vs > RTC_AREA_MAX_SAMPLES)
        throw Error("Overflow", "area-light: more than 4096 samples");
      Light light;
      light.kind = RTC_LIGHT_AREA;
      light.corner = Tuple::point(corner[0], corner[1], corner[2]);
      light.uvec = Tuple::vec3(u[0], u[1], u[2]);
      light.vvec = Tuple::vec3(v[0], v[1], v[2]);
      light.usteps = static_cast<uint32_t>(us);
      light.vsteps = static_cast<uint32_t>(vs);
      const Value* jitter = cfg.find("jitter");  // (optional: false)
      light.jitter = jitter ? asBool(*jitter, "jitter") : false;
      light.position = Tuple::point((corner[0] + u[0] * 0.5) + v[0] * 0.5, (corner[1] + u[1] * 0.5) + v[1] * 0.5,
                                    (corner[2] + u[2] * 0.5) + v[2] * 0.5);
      light.intensity = {c[0], c[1], c[2]};
      info.world.lights.push_back(light);
      info.spots.emplace_back();
      continue;
    }
    if (kv.first == "spot-light") {  // (not in the reference): a point light that shines into a cone
      const Value& cfg = requireObject(kv.second, "spot-light");
      checkFields(cfg, {"position", "intensity", "to", "direction", "outer-angle", "inner-angle"}, "spot-light");
      // (an entry that names no cone at all is refused as the light kind this loader did not know before spot lights)
      if (!cfg.find("to") && !cfg.find("direction") && !cfg.find("outer-angle"))
        throw Error("UnknownField", "light.spot-light: a spot-light names its cone (\"to\" or \"direction\", and \"outer-angle\")");
      double p[3], c[3], a[3];
      asVec3(requireField(cfg, "position", "spot-light"), "position", p);
      asVec3(requireField(cfg, "intensity", "spot-light"), "intensity", c);
      const Value* to = cfg.find("to");
      const Value* direction = cfg.find("direction");
      if ((to != nullptr) == (direction != nullptr)) throw Error("InvalidData", "spot-light: exactly one of \"to\" and \"direction\"");
      if (to) {
        double t[3];
        asVec3(*to, "to", t);
        for (int k = 0; k < 3; ++k) a[k] = t[k] - p[k];
      } else {
        asVec3(*direction, "direction", a);
      }
      const double mag = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);  // (the library normalizes it so)
      if (!(std::isfinite(mag) && mag > 0.0))
        throw Error("InvalidData", to ? "spot-light.to: a point other than position, at a finite distance"
                                      : "spot-light.direction: a finite vector other than zero");
      for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p[k])) throw Error("InvalidData", "spot-light.position: every component is finite");
      const double pi = std::acos(-1.0);
      const double outer = asFloat(requireField(cfg, "outer-angle", "spot-light"), "outer-angle");
      if (!(outer > 0.0 && outer <= pi)) throw Error("InvalidData", "spot-light.outer-angle: a half-angle in (0, pi] radians");
      double inner = outer;  // (optional: a hard edge)
      if (const Value* in = cfg.find("inner-angle")) {
        inner = asFloat(*in, "inner-angle");
        if (!(inner >= 0.0 && inner <= outer)) throw Error("InvalidData", "spot-light.inner-angle: a half-angle in [0, outer-angle] radians");
      }
      info.world.lights.push_back({Tuple::point(p[0], p[1], p[2]), {c[0], c[1], c[2]}});
      SpotCone cone;
      cone.cone = 1;
      for (int k = 0; k < 3; ++k) cone.axis[k] = a[k];
      cone.cos_inner = std::cos(inner);
      cone.cos_outer = std::cos(outer);
      info.spots.push_back(cone);
      continue;
    }
    if (kv.first != "point-light") throw Error("UnknownField", "light." + kv.first);
    const Value& cfg = requireObject(kv.second, "point-light");
    checkFields(cfg, {"position", "intensity"}, "point-light");
    double p[3], c[3];
    asVec3(requireField(cfg, "position", "point-light"), "position", p);
    asVec3(requireField(cfg, "intensity", "point-light"), "intensity", c);
    info.world.lights.push_back({Tuple::point(p[0], p[1], p[2]), {c[0], c[1], c[2]}});
    info.spots.emplace_back();
  }
  return info;
}

// =========================================================================================
// OBJ parser, obj.zig
// =========================================================================================
namespace {

// std.mem.tokenizeScalar: split on ONE delimiter byte, empty tokens skipped.  Tokens are views into the text (an OBJ
// file is a few hundred thousand of them: no allocation per token).
using Token = std::string_view;
void tokenize(Token s, char delim, std::vector<Token>& out) {
  out.clear();
  size_t i = 0;
  while (i < s.size()) {
    while (i < s.size() && s[i] == delim) ++i;
    size_t j = i;
    while (j < s.size() && s[j] != delim) ++j;
    if (j > i) out.push_back(s.substr(i, j - i));
    i = j;
  }
}

struct LineError {  // an error from the ObjParser.Error set or from parseFloat/parseInt
  const char* name;
};

double parseFloatToken(Token tok) {  // std.fmt.parseFloat: whole token, no whitespace
  if (tok.empty() || std::isspace(static_cast<unsigned char>(tok[0]))) throw LineError{"InvalidCharacter"};
  char small[64];
  std::string big;
  const char* text = small;
  if (tok.size() < sizeof small) {  // strtod wants a terminated string
    std::memcpy(small, tok.data(), tok.size());
    small[tok.size()] = '\0';
  } else {
    big.assign(tok);
    text = big.c_str();
  }
  errno = 0;
  char* end = nullptr;
  const double v = std::strtod(text, &end);
  if (end != text + tok.size()) throw LineError{"InvalidCharacter"};
  return v;
}

size_t parseUsizeToken(Token tok) {  // std.fmt.parseInt(usize, tok, 10)
  size_t i = 0;
  if (i < tok.size() && tok[i] == '+') ++i;
  if (i >= tok.size()) throw LineError{"InvalidCharacter"};
  size_t v = 0;
  for (; i < tok.size(); ++i) {
    const char c = tok[i];
    if (c < '0' || c > '9') throw LineError{"InvalidCharacter"};
    const size_t nv = v * 10 + static_cast<size_t>(c - '0');
    if (nv < v) throw LineError{"Overflow"};
    v = nv;
  }
  return v;
}

struct FaceVertex {
  size_t vertex_index;
  std::optional<size_t> normal_index;
  std::optional<size_t> texture_index;  // (only with "texture-coordinates")
};

// obj.zig:85-99 — "v", "v/t", "v/t/n", "v//n".  `with_texture`: the t field too, where it is there and not empty.
FaceVertex handleFaceHelper(Token token, bool with_texture) {
  // std.mem.splitScalar keeps empty fields: field 0 is the vertex, field 2 (if there is one) the normal.
  Token parts[3];
  size_t n_parts = 0, start = 0;
  while (true) {
    const size_t p = token.find('/', start);
    const Token part = p == Token::npos ? token.substr(start) : token.substr(start, p - start);
    if (n_parts < 3) parts[n_parts] = part;
    ++n_parts;
    if (p == Token::npos) break;
    start = p + 1;
  }
  FaceVertex fv;
  fv.vertex_index = parseUsizeToken(parts[0]);
  if (with_texture && n_parts >= 2 && !parts[1].empty()) fv.texture_index = parseUsizeToken(parts[1]);
  if (n_parts < 3) return fv;  // no texture field, or no normal field
  fv.normal_index = parseUsizeToken(parts[2]);
  return fv;
}

}  // namespace

ObjParser::ObjParser() : default_group(Shape::group()) {}

void ObjParser::handleLine(std::string_view line, const InheritedState& state) {
  std::vector<Token>& tokens = line_tokens_;
  tokenize(line, ' ', tokens);
  if (tokens.empty()) throw LineError{"LineEmpty"};
  const Token first = tokens[0];
  auto tok = [&](size_t i, const char* err) -> Token {
    if (i >= tokens.size()) throw LineError{err};
    return tokens[i];
  };
  if (first == "v") {  // obj.zig:53-68
    const double x = parseFloatToken(tok(1, "IncompleteVertex"));
    const double y = parseFloatToken(tok(2, "IncompleteVertex"));
    const double z = parseFloatToken(tok(3, "IncompleteVertex"));
    // offset is a vector (w=0), so a normalised vertex carries w = 1/scale (obj.zig:66).
    vertices.push_back(Tuple::point(x, y, z).sub(offset).div(scale));
  } else if (first == "vn") {  // obj.zig:70-83
    const double x = parseFloatToken(tok(1, "IncompleteVertex"));
    const double y = parseFloatToken(tok(2, "IncompleteVertex"));
    const double z = parseFloatToken(tok(3, "IncompleteVertex"));
    normals.push_back(Tuple::vec3(x, y, z));
  } else if (first == "vt" && texture_coordinates) {  // vt u v [w]: w is not read
    const double u = parseFloatToken(tok(1, "IncompleteVertex"));
    const double v = parseFloatToken(tok(2, "IncompleteVertex"));
    if (!std::isfinite(u) || !std::isfinite(v)) throw LineError{"NonFiniteVertex"};  // (rtc_scene_set_mesh_uvs takes finite rows only)
    texcoords.emplace_back(u, v);
  } else if (first == "f") {  // obj.zig:101-150 — fan triangulation
    const FaceVertex firstv = handleFaceHelper(tok(1, "IncompleteFace"), texture_coordinates);
    FaceVertex last = handleFaceHelper(tok(2, "IncompleteFace"), texture_coordinates);
    if (tokens.size() < 4) throw LineError{"IncompleteFace"};
    auto vertexAt = [&](size_t idx) -> const Tuple& {
      if (idx == 0 || idx > vertices.size()) throw Error("IndexOutOfBounds", "face vertex " + std::to_string(idx));
      return vertices[idx - 1];  // 1-indexed
    };
    auto normalAt = [&](size_t idx) -> const Tuple& {
      if (idx == 0 || idx > normals.size()) throw Error("IndexOutOfBounds", "face normal " + std::to_string(idx));
      return normals[idx - 1];
    };
    auto texAt = [&](const FaceVertex& fv, double* out) {  // a vertex without a t field: (0, 0)
      out[0] = out[1] = 0.0;
      if (!fv.texture_index) return;
      const size_t idx = *fv.texture_index;
      if (idx == 0 || idx > texcoords.size()) throw Error("IndexOutOfBounds", "face texture " + std::to_string(idx));
      out[0] = texcoords[idx - 1].first;  // 1-indexed
      out[1] = texcoords[idx - 1].second;
    };
    for (size_t i = 3; i < tokens.size(); ++i) {
      const FaceVertex current = handleFaceHelper(tokens[i], texture_coordinates);
      const Tuple& p1 = vertexAt(firstv.vertex_index);
      const Tuple& p2 = vertexAt(last.vertex_index);
      const Tuple& p3 = vertexAt(current.vertex_index);
      Shape tri = (firstv.normal_index && last.normal_index && current.normal_index)
                      ? Shape::smoothTriangle(p1, p2, p3, normalAt(*firstv.normal_index), normalAt(*last.normal_index),
                                              normalAt(*current.normal_index))
                      : Shape::triangle(p1, p2, p3);
      if (texture_coordinates) {  // the fan's firstv, last, current
        texAt(firstv, tri.tex_uv + 0);
        texAt(last, tri.tex_uv + 2);
        texAt(current, tri.tex_uv + 4);
      }
      tri.material = state.material ? *state.material : Material{};  // copied into EVERY triangle
      tri.casts_shadow = state.casts_shadow ? *state.casts_shadow : true;
      activeGroup().addChild(std::move(tri));
      last = current;
    }
  } else if (first == "g") {  // obj.zig:152-169
    const std::string name(tok(1, "IncompleteNamedGroup"));
    default_group.addChild(Shape::group());
    active_group_ = static_cast<long>(default_group.children.size()) - 1;
    named_groups[name] = static_cast<size_t>(active_group_);
  } else {
    throw LineError{"UnknownFirstToken"};
  }
}

void ObjParser::loadObj(const std::string& obj, const InheritedState& state, bool normalize) {
  std::vector<Token> lines;
  tokenize(obj, '\n', lines);  // empty lines are skipped, never "ignored"

  if (normalize) {  // obj.zig:198-271
    double min_x = kInf, min_y = kInf, min_z = kInf;
    double max_x = -kInf, max_y = -kInf, max_z = -kInf;
    std::vector<Token> tokens;
    for (const Token line : lines) {
      tokenize(line, ' ', tokens);
      if (tokens.empty() || tokens[0] != "v") continue;
      auto coord = [&](size_t i) -> std::optional<double> {
        if (i >= tokens.size()) return std::nullopt;
        try {
          return parseFloatToken(tokens[i]);
        } catch (const LineError&) {
          return std::nullopt;
        }
      };
      if (auto x = coord(1)) {
        if (*x < min_x) min_x = *x;
        if (*x > max_x) max_x = *x;
      }
      if (auto y = coord(2)) {
        if (*y < min_y) min_y = *y;
        if (*y > max_y) max_y = *y;
      }
      if (auto z = coord(3)) {
        if (*z < min_z) min_z = *z;
        if (*z > max_z) max_z = *z;
      }
    }
    const double sx = max_x - min_x, sy = max_y - min_y, sz = max_z - min_z;
    const double x_offset = min_x + 0.5 * sx;
    const double y_offset = min_y + 0.5 * sy;
    const double z_offset = min_z + 0.5 * sz;
    const double scale_ = 0.5 * std::fmax(sx, std::fmax(sy, sz));
    offset = Tuple::vec3(x_offset, y_offset, z_offset);
    scale = scale_;
  }

  for (const Token line : lines) {
    try {
      handleLine(line, state);
    } catch (const LineError& e) {
      lines_ignored += 1;  // obj.zig:277
      ignored_by_error[e.name] += 1;
    }
  }
}

}  // namespace rtc
