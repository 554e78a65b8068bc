// Scene.cpp — procedural scenes with the reference's content (CudaTracer/Scene.cpp:17-371),
// written table-first: every box is a list of {placement, material slot} rows fed to one helper.
// Numbers (colours, exponents, IORs, wall angles, light powers) are the reference's data and are
// cited per block; the code that assembles them is this repo's own.
#include "Scene.h"

#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <array>
#include <map>
#include <sstream>

namespace {

const vec3 kAxisX = {1, 0, 0};
const vec3 kAxisY = {0, 1, 0};

struct WallRow {
    vec3 shift;     // translate(...)
    float degrees;  // rotate(degrees, axis); 0 = no rotation factor
    vec3 axis;
    float edge;     // uniform scale
    int slot;       // material slot relative to the box's first material
};

mat4 place(const WallRow& w) {
    mat4 m = translate(w.shift);
    if (w.degrees != 0.0f) m = m * rotate(w.degrees, w.axis);
    return m * scale(v3(w.edge));
}

// glass: white diffuse colour with zero diffuse weight, white mirror-like specular (exponent inf),
// specAvg/refrAvg 0.7, IOR 1.55, coloured absorption           (reference Scene.cpp:128-140)
Material glass(vec3 absorption) {
    return Material(v3(1.0f), 0.0f, v3(1.0f), PTSS_INFINITY, 0.7f, 1.55f, absorption, 0.7f);
}

// Cook-Torrance lobe: diffAvg .1, specAvg .6, IOR 1.7, exponent inf (reference Scene.cpp:198-210)
Material cookTorrance(vec3 diffuse, vec3 specular, float roughness) {
    Material m(diffuse, 0.1f, specular, PTSS_INFINITY, 0.6f, 1.7f);
    m.flags |= MAT_FLAG_COOK_TORRANCE;
    m.roughness = roughness;
    return m;
}

}  // namespace

Scene::Scene() {}
Scene::~Scene() {}

// rand() of the reference is MSVC v120's, unseeded (Scene.cpp:3, CudaTracer.vcxproj): the LCG below with RAND_MAX =
// 32767 [unverifiable offline]. UNPINNED ASSUMPTION beside it: the reference draws a sphere's coordinates as constructor
// ARGUMENTS — vec3(rnd(5.0f) - 2.5f, rnd(5.0f) - 2.5f, rnd(7.0f) - 9.0f) (Scene.cpp:161, 219) — and C++ leaves the
// evaluation order of function arguments unspecified (MSVC commonly evaluates them right to left). The generators here
// draw x, then y, then z (left to right), so the "same spheres every time" layout of the default / mixed / lambert
// presets is self-consistent but may be the reference's with x and z draws swapped (`positionDrawsRightToLeft`, preset
// suffix "@rtl", builds that other layout); nothing the reference holds can decide it (its image.tga shows the defined spheres of the Cornell preset, which draw nothing). Statistically the two
// layouts are the same scene: 20 spheres of the same size distribution in the same box.
int Scene::nextRand() {
    randState = randState * 214013u + 2531011u;
    return (int)((randState >> 16) & 0x7fffu);
}
// `#define rnd(x) (x * rand() / RAND_MAX)` with a float x (Scene.cpp:3): float*int, then /int.
float Scene::rnd(float x) { return x * (float)nextRand() / (float)32767; }
// `rnd(1);` statements (Scene.cpp:159,217) are integer expressions whose only effect is a draw.
void Scene::burn(int draws) {
    for (int i = 0; i < draws; ++i) (void)nextRand();
}

// Scene.cpp:17-32 — the code's default: 5 Cook-Torrance + 15 glass spheres in a 10-unit mirror box.
void Scene::build() {
    addRandomSpheres(5);
    addRandomGlassSpheres(15);
    addMirrorBox(10);
}

// Scene.cpp:63-96 — unit square in z=0 pushed through `transformation`; two triangles
// (v0,v1,v2),(v3,v1,v2) sharing one flat normal = normalize(inverse(transpose(M)) * (0,0,1,0)).
void Scene::addRectangularModel(mat4 transformation, int materialIdx) {
    vec3 corner[4];
    for (int k = 0; k < 4; ++k) {
        const vec4 p = transformation * vec4{(float)(k >> 1) - 0.5f, (float)(k & 1) - 0.5f, 0.0f, 1.0f};
        corner[k] = v3(p.x, p.y, p.z);
    }
    const vec4 n4 = inverse(transpose(transformation)) * vec4{0.0f, 0.0f, 1.0f, 0.0f};
    const vec3 n = ptv::normalize(v3(n4.x, n4.y, n4.z));
    trianglesVec.push_back(Triangle(corner[0], corner[1], corner[2], n, n, n, materialIdx));
    trianglesVec.push_back(Triangle(corner[3], corner[1], corner[2], n, n, n, materialIdx));
}

// Scene.cpp:40-55 — rectangle + AreaLight{power, first triangle index, 2, |e1 x e2|}.
void Scene::addAreaLight(mat4 transformation, int materialIdx, vec3 power) {
    using namespace ptv;
    const size_t first = trianglesVec.size();
    addRectangularModel(transformation, materialIdx);
    const Triangle& t = trianglesVec[first];
    const vec3 e1 = t.vertex1 - t.vertex2;
    const vec3 e2 = t.vertex2 - t.vertex0;
    areaLightsVec.push_back(AreaLight(power, (int)first, 2, length(cross(e1, e2))));
}

// Scene.cpp:98-109 — one Phong-glass (exponent 300) and one red Phong (exponent 250) sphere.
void Scene::addDefinedSpheres(const float size) {
    const int first = (int)materialsVec.size();
    materialsVec.push_back(Material(v3(1.0f, 0.0f, 0.0f), 0.35f, v3(1.0f), 250, 0.6f, 2.5f));
    materialsVec.push_back(Material(v3(1.0f), 0.0f, v3(1.0f), 300, 0.9f, 1.55f, v3(0.15f, 0.15f, 0.0f), 0.9f));
    spheresVec.push_back(Sphere(v3(-2, -(size - 1.5f), -(size * 1.3f)), 1.5f, first + 1));
    spheresVec.push_back(Sphere(v3(1, -(size - 1.0f), -(size * 1.4f)), 1.0f, first));
}

// Scene.cpp:115-167 — three absorbing glasses; per sphere 3 burnt draws, then x,y,z,radius.
void Scene::addRandomGlassSpheres(const size_t numSpheres) {
    const int first = (int)materialsVec.size();
    materialsVec.push_back(glass(v3(0.0f, 0.75f, 0.75f)));  // "red glass" (absorbs G,B)
    materialsVec.push_back(glass(v3(0.75f, 0.75f, 0.0f)));  // "blue glass"
    materialsVec.push_back(glass(v3(0.75f, 0.0f, 0.75f)));  // "green glass"
    for (size_t i = 0; i < numSpheres; ++i) {
        burn(3);
        float x, y, z;
        if (positionDrawsRightToLeft) {  // the other legal order of vec3(...)'s arguments (see nextRand)
            z = rnd(7.0f) - 9.0f;
            y = rnd(5.0f) - 2.5f;
            x = rnd(5.0f) - 2.5f;
        } else {
            x = rnd(5.0f) - 2.5f;
            y = rnd(5.0f) - 2.5f;
            z = rnd(7.0f) - 9.0f;
        }
        const float r = rnd(1.0f) + 0.2f;
        spheresVec.push_back(Sphere(v3(x, y, z), r, first + (int)(i % 3)));
    }
}

// Scene.cpp:173-225 — three Cook-Torrance materials; per sphere 2 burnt draws, then x,y,z,radius.
void Scene::addRandomSpheres(const size_t numSpheres) {
    const int first = (int)materialsVec.size();
    materialsVec.push_back(cookTorrance(v3(1.0f, 0.1f, 0.1f), v3(1.0f, 0.2f, 0.2f), 0.3f));
    materialsVec.push_back(cookTorrance(v3(0.1f, 0.1f, 1.0f), v3(0.2f, 0.2f, 1.0f), 0.1f));
    materialsVec.push_back(cookTorrance(v3(0.1f, 1.0f, 0.1f), v3(0.2f, 1.0f, 0.2f), 0.5f));
    for (size_t i = 0; i < numSpheres; ++i) {
        burn(2);
        float x, y, z;
        if (positionDrawsRightToLeft) {  // the other legal order of vec3(...)'s arguments (see nextRand)
            z = rnd(7.0f) - 9.0f;
            y = rnd(5.0f) - 2.5f;
            x = rnd(5.0f) - 2.5f;
        } else {
            x = rnd(5.0f) - 2.5f;
            y = rnd(5.0f) - 2.5f;
            z = rnd(7.0f) - 9.0f;
        }
        const float r = rnd(1.0f) + 0.2f;
        spheresVec.push_back(Sphere(v3(x, y, z), r, first + (int)(i % 3)));
    }
}

// Scene.cpp:231-294 — open-front box: white floor/ceiling/back, red left, green right, a mirror
// panel (specAvg .8, IOR 5.8, no PURE_REFLECTION flag) just inside the right wall, 2.5^2 ceiling light 400.
void Scene::addCornellBox(const float wallSize) {
    const int first = (int)materialsVec.size();
    materialsVec.push_back(Material(v3(1.0f, 1.0f, 0.8f), 0.7f));                                   // +0 white
    materialsVec.push_back(Material(v3(1.0f, 0.0f, 0.0f), 0.7f));                                   // +1 red
    materialsVec.push_back(Material(v3(0.0f, 1.0f, 0.0f), 0.7f));                                   // +2 green
    materialsVec.push_back(Material(v3(1.0f, 1.0f, 1.0f)));                                         // +3 emitter
    materialsVec.push_back(Material(v3(0.0f), 0.0f, v3(1.0f), PTSS_INFINITY, 0.8f, 5.8f));          // +4 mirror

    const float h = wallSize / 2;
    const WallRow walls[] = {
        {v3(0, -h, -h), -90.0f, kAxisX, wallSize, 0},              // floor
        {v3(0, h, -h), 90.0f, kAxisX, wallSize, 0},                // ceiling
        {v3(-h, 0, -h), 90.0f, kAxisY, wallSize, 1},               // left
        {v3(h, 0, -h), -90.0f, kAxisY, wallSize, 2},               // right
        {v3(h - 0.02f, 0, -h), -90.0f, kAxisY, wallSize - 2, 4},   // mirror panel
        {v3(0, 0, -wallSize), 0.0f, kAxisY, wallSize, 0},          // back
    };
    for (const WallRow& w : walls) addRectangularModel(place(w), first + w.slot);

    const float power = 400;
    addAreaLight(place({v3(0, h - 0.01f, -h), 90.0f, kAxisX, 2.5f, 3}), first + 3, v3(power));
}

// Scene.cpp:301-371 — closed box: white floor/back/front, PURE_REFLECTION mirror (specAvg .9,
// IOR 5.8) on ceiling, right and an 88-degree left wall pulled in by 0.2*offset; ceiling light
// (100,400,400) 2.5^2 and a floor light (133.3,0,133.3) 1.5^2 with a violet emitter material.
void Scene::addMirrorBox(const float wallSize) {
    const int first = (int)materialsVec.size();
    materialsVec.push_back(Material(v3(1.0f, 1.0f, 0.8f), 0.7f));                                   // +0 white
    materialsVec.push_back(Material(v3(1.0f, 0.0f, 0.0f), 0.7f));                                   // +1 red (unused)
    materialsVec.push_back(Material(v3(0.0f, 1.0f, 0.0f), 0.7f));                                   // +2 green (unused)
    materialsVec.push_back(Material(v3(1.0f, 1.0f, 1.0f)));                                         // +3 white emitter
    Material mirror(v3(0.0f), 0.0f, v3(1.0f), PTSS_INFINITY, 0.9f, 5.8f);                           // +4 mirror
    mirror.flags |= MAT_FLAG_PURE_REFLECTION;
    materialsVec.push_back(mirror);
    materialsVec.push_back(Material(v3(1.0f, 0.6f, 1.0f)));                                         // +5 violet emitter

    const float h = wallSize / 2;
    // `-offset + .2 * offset` is evaluated in double in the reference and narrowed by vec3's ctor
    const float leftX = (float)(-(double)h + 0.2 * (double)h);
    const WallRow walls[] = {
        {v3(0, -h, -h), -90.0f, kAxisX, wallSize, 0},      // floor
        {v3(0, h, -h), 90.0f, kAxisX, wallSize, 4},        // ceiling (mirror)
        {v3(leftX, 0, -h), 88.0f, kAxisY, wallSize, 4},    // left (mirror, 88 degrees)
        {v3(h, 0, -h), -90.0f, kAxisY, wallSize, 4},       // right (mirror)
        {v3(0, 0, -wallSize), 0.0f, kAxisY, wallSize, 0},  // back
        {v3(0, 0, 0), 180.0f, kAxisY, wallSize, 0},        // front, through the camera plane
    };
    for (const WallRow& w : walls) addRectangularModel(place(w), first + w.slot);

    const float power = 400;
    addAreaLight(place({v3(0, h - 0.01f, -h), 90.0f, kAxisX, 2.5f, 3}), first + 3, v3(power / 4, power, power));
    addAreaLight(place({v3(0, -h + 0.01f, -h), -90.0f, kAxisX, 1.5f, 5}), first + 5, v3(power / 3, 0, power / 3));
}

// ------------------------------------------------------------------------------------------------
// Additions (not in the reference): presets for BASELINE.json's five configs, SURVEY.md §9.6.
// ------------------------------------------------------------------------------------------------

// n spheres, uniformly placed in [-halfXY,halfXY]^2 x [zFar,zNear], radius in [rMin,rMax], cycling
// through every material present when called. Same draw discipline as addRandomSpheres.
void Scene::addSphereField(size_t numSpheres, float halfXY, float zNear, float zFar, float rMin, float rMax) {
    const int numMaterials = (int)materialsVec.size();
    for (size_t i = 0; i < numSpheres; ++i) {
        burn(2);
        const float x = rnd(2 * halfXY) - halfXY;
        const float y = rnd(2 * halfXY) - halfXY;
        const float z = rnd(zNear - zFar) + zFar;
        const float r = rnd(rMax - rMin) + rMin;
        spheresVec.push_back(Sphere(v3(x, y, z), r, numMaterials ? (int)(i % (size_t)numMaterials) : 0));
    }
}

// C2: every non-emissive material becomes Material(colour, 0.7f) — pure Lambert.
void Scene::makeLambertOnly() {
    for (Material& m : materialsVec) {
        const bool emits = m.emmitance.x > 0 || m.emmitance.y > 0 || m.emmitance.z > 0;
        if (emits) continue;
        const bool hasDiffuse = m.diffuseColor.x > 0 || m.diffuseColor.y > 0 || m.diffuseColor.z > 0;
        m = Material(hasDiffuse ? m.diffuseColor : m.specularColor, 0.7f);
    }
}

bool Scene::buildPreset(const std::string& preset) {
    // "<name>@rtl": the reference's random-sphere generators with their position arguments drawn right to left
    std::string name = preset;
    positionDrawsRightToLeft = false;   // a property of THIS build, not of the object: a later preset without the suffix draws left to right again
    const size_t at = name.find("@rtl");
    if (at != std::string::npos && at + 4 == name.size()) {
        positionDrawsRightToLeft = true;
        name.erase(at);
    }
    if (name == "default") {  // C1 literal default, also the geometry of C2
        build();
    } else if (name == "cornell") {  // C1 as BASELINE words it; matches CudaTracer/image.tga
        addDefinedSpheres(4);
        addCornellBox(8);
    } else if (name == "lambert") {  // C2
        build();
        makeLambertOnly();
    } else if (name == "mixed") {  // C3/C4: default + the two finite-exponent Phong spheres
        addRandomSpheres(5);
        addRandomGlassSpheres(15);
        addDefinedSpheres(4);
        addMirrorBox(10);
    } else if (name == "stress") {  // C5: 1,024 spheres of every material class in an open box
        materialsVec.push_back(cookTorrance(v3(1.0f, 0.1f, 0.1f), v3(1.0f, 0.2f, 0.2f), 0.3f));
        materialsVec.push_back(glass(v3(0.0f, 0.75f, 0.75f)));
        materialsVec.push_back(Material(v3(0.2f, 0.4f, 1.0f), 0.7f));
        materialsVec.push_back(Material(v3(1.0f, 0.0f, 0.0f), 0.35f, v3(1.0f), 250, 0.6f, 2.5f));
        addSphereField(1024, 3.6f, -1.5f, -7.7f, 0.05f, 0.22f);
        addCornellBox(8);
    } else if (name == "mesh") {  // a model instead of the two spheres: a level-4 icosphere (5,120 triangles) in Cook-Torrance
        addCornellBox(8);
        materialsVec.push_back(cookTorrance(v3(0.9f, 0.6f, 0.2f), v3(1.0f, 0.8f, 0.4f), 0.2f));
        addIcosphere(v3(0.5f, -2.5f, -5.5f), 1.5f, 4, (int)materialsVec.size() - 1);
    } else if (name == "pointlight") {  // §8f-3: the commented-out point lights of Scene.cpp:21-22
        addDefinedSpheres(4);
        addCornellBox(8);
        areaLightsVec.clear();
        const float power = 500;
        pointLightsVec.push_back(PointLight(v3(0, 0.0f, 2.5f), v3(power)));
        pointLightsVec.push_back(PointLight(v3(2, 3.0f, -5), v3(power)));
    } else {
        return false;
    }
    return true;
}

ptss_scene_desc Scene::desc(vec3 defaultColor) const {
    ptss_scene_desc d{};
    d.spheres = spheresVec.data();
    d.numSpheres = spheresVec.size();
    d.triangles = trianglesVec.data();
    d.numTriangles = trianglesVec.size();
    d.materials = materialsVec.data();
    d.numMaterials = materialsVec.size();
    d.pointLights = pointLightsVec.data();
    d.numPointLights = pointLightsVec.size();
    d.areaLights = areaLightsVec.data();
    d.numAreaLights = areaLightsVec.size();
    d.defaultColor = defaultColor;
    return d;
}

// ------------------------------------------------------------------------------------------------
// Meshes (not in the reference, whose README names OBJ support as its next feature).
// ------------------------------------------------------------------------------------------------

namespace {

bool parseFloat(const std::string& tok, float& out) {
    if (tok.empty()) return false;
    const char* b = tok.c_str();
    char* e = nullptr;
    errno = 0;
    const float v = std::strtof(b, &e);
    if (e != b + tok.size() || !std::isfinite(v)) return false;
    out = v;
    return true;
}

// an OBJ index: 1-based, or negative = relative to the `count` elements read so far; false if malformed or out of range
bool parseIndex(const std::string& tok, size_t count, size_t& out) {
    if (tok.empty()) return false;
    const char* b = tok.c_str();
    char* e = nullptr;
    errno = 0;
    const long long v = std::strtoll(b, &e, 10);
    if (e != b + tok.size() || errno != 0 || v == 0) return false;
    const long long idx = v > 0 ? v - 1 : (long long)count + v;
    if (idx < 0 || idx >= (long long)count) return false;
    out = (size_t)idx;
    return true;
}

vec3 transformPoint(const mat4& m, vec3 p) {
    const vec4 q = m * vec4{p.x, p.y, p.z, 1.0f};
    return v3(q.x, q.y, q.z);
}

vec3 safeNormalize(vec3 n) {   // a degenerate face keeps a zero normal instead of NaNs
    const float len2 = ptv::dot(n, n);
    return len2 > 0.0f ? ptv::normalize(n) : v3(0, 0, 0);
}

}  // namespace

long Scene::addObjText(const std::string& text, mat4 transformation, int materialIdx, std::string* error) {
    using namespace ptv;
    std::vector<vec3> positions, normals;
    size_t texcoords = 0;
    std::vector<Triangle> added;
    const mat4 normalMatrix = inverse(transpose(transformation));
    std::istringstream lines(text);
    std::string line;
    size_t lineNo = 0;
    auto fail = [&](const std::string& why) -> long {
        if (error) *error = "line " + std::to_string(lineNo) + ": " + why;
        return -1;
    };
    while (std::getline(lines, line)) {
        ++lineNo;
        if (!line.empty() && line.back() == '\r') line.pop_back();   // CRLF files
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.erase(hash);
        std::istringstream words(line);
        std::string key;
        if (!(words >> key)) continue;   // blank or comment
        std::vector<std::string> args;
        for (std::string w; words >> w;) args.push_back(w);
        if (key == "v" || key == "vn") {
            // v x y z [w] (w is ignored: no rational curves here); vn x y z
            if (args.size() < 3 || args.size() > (key == "v" ? 4u : 3u)) return fail("expected three coordinates after '" + key + "'");
            float c[4];
            for (size_t k = 0; k < args.size(); ++k)
                if (!parseFloat(args[k], c[k])) return fail("not a finite number: '" + args[k] + "'");
            (key == "v" ? positions : normals).push_back(v3(c[0], c[1], c[2]));
        } else if (key == "vt") {
            ++texcoords;   // counted so that a face's texture indices can be range-checked; the coordinates are not used
        } else if (key == "f") {
            if (args.size() < 3) return fail("a face needs at least three vertices");
            std::vector<size_t> vi(args.size()), ni(args.size());
            bool allNormals = true;
            for (size_t k = 0; k < args.size(); ++k) {
                // i, i/j, i//k, i/j/k
                const std::string& a = args[k];
                const size_t s1 = a.find('/');
                const size_t s2 = s1 == std::string::npos ? std::string::npos : a.find('/', s1 + 1);
                if (s2 != std::string::npos && a.find('/', s2 + 1) != std::string::npos) return fail("bad face vertex '" + a + "'");
                if (!parseIndex(a.substr(0, s1), positions.size(), vi[k])) return fail("vertex index out of range or malformed in '" + a + "'");
                if (s1 != std::string::npos) {
                    const std::string t = a.substr(s1 + 1, s2 == std::string::npos ? std::string::npos : s2 - s1 - 1);
                    size_t unused;
                    if (!(t.empty() && s2 != std::string::npos) && !parseIndex(t, texcoords, unused))
                        return fail("texture index out of range or malformed in '" + a + "'");
                }
                if (s2 != std::string::npos) {
                    if (!parseIndex(a.substr(s2 + 1), normals.size(), ni[k])) return fail("normal index out of range or malformed in '" + a + "'");
                } else {
                    allNormals = false;
                }
            }
            for (size_t k = 1; k + 1 < args.size(); ++k) {   // fan: (0, k, k + 1)
                const size_t c[3] = {0, k, k + 1};
                vec3 p[3], n[3];
                for (int j = 0; j < 3; ++j) p[j] = transformPoint(transformation, positions[vi[c[j]]]);
                if (allNormals) {
                    for (int j = 0; j < 3; ++j) {
                        const vec3 m = normals[ni[c[j]]];
                        const vec4 q = normalMatrix * vec4{m.x, m.y, m.z, 0.0f};
                        n[j] = safeNormalize(v3(q.x, q.y, q.z));
                    }
                } else {
                    n[0] = n[1] = n[2] = safeNormalize(ptv::cross(p[1] - p[0], p[2] - p[0]));
                }
                added.push_back(Triangle(p[0], p[1], p[2], n[0], n[1], n[2], materialIdx));
            }
        } else if (key == "o" || key == "g" || key == "s" || key == "usemtl" || key == "mtllib") {
            // grouping, smoothing and material statements: the whole model wears materialIdx
        } else {
            return fail("unsupported statement '" + key + "'");
        }
    }
    trianglesVec.insert(trianglesVec.end(), added.begin(), added.end());
    return (long)added.size();
}

long Scene::addObjModel(const std::string& path, mat4 transformation, int materialIdx, std::string* error) {
    std::ifstream in(path, std::ios::binary);
    if (!in) {
        if (error) *error = "cannot open " + path;
        return -2;
    }
    std::ostringstream text;
    text << in.rdbuf();
    if (in.bad()) {
        if (error) *error = "cannot read " + path;
        return -2;
    }
    return addObjText(text.str(), transformation, materialIdx, error);
}

void Scene::addIcosphere(vec3 centre, float radius, int level, int materialIdx) {
    using namespace ptv;
    const double g = (1 + std::sqrt(5.0)) / 2;
    std::vector<std::array<double, 3>> verts = {{-1, g, 0}, {1, g, 0}, {-1, -g, 0}, {1, -g, 0}, {0, -1, g}, {0, 1, g},
                                                {0, -1, -g}, {0, 1, -g}, {g, 0, -1}, {g, 0, 1}, {-g, 0, -1}, {-g, 0, 1}};
    std::vector<std::array<int, 3>> faces = {{0, 11, 5}, {0, 5, 1}, {0, 1, 7}, {0, 7, 10}, {0, 10, 11}, {1, 5, 9}, {5, 11, 4},
                                             {11, 10, 2}, {10, 7, 6}, {7, 1, 8}, {3, 9, 4}, {3, 4, 2}, {3, 2, 6}, {3, 6, 8},
                                             {3, 8, 9}, {4, 9, 5}, {2, 4, 11}, {6, 2, 10}, {8, 6, 7}, {9, 8, 1}};
    auto unit = [](std::array<double, 3> p) {
        const double l = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
        return std::array<double, 3>{p[0] / l, p[1] / l, p[2] / l};
    };
    for (auto& v : verts) v = unit(v);
    for (int l = 0; l < level; ++l) {
        std::map<std::pair<int, int>, int> mid;   // one midpoint per edge, so that neighbours share their vertices exactly
        auto midpoint = [&](int a, int b) {
            const std::pair<int, int> key(a < b ? a : b, a < b ? b : a);
            auto it = mid.find(key);
            if (it != mid.end()) return it->second;
            const auto& p = verts[(size_t)key.first];
            const auto& q = verts[(size_t)key.second];
            verts.push_back(unit({p[0] + q[0], p[1] + q[1], p[2] + q[2]}));
            return mid[key] = (int)verts.size() - 1;
        };
        std::vector<std::array<int, 3>> next;
        for (const auto& f : faces) {
            const int a = midpoint(f[0], f[1]), b = midpoint(f[1], f[2]), c = midpoint(f[2], f[0]);
            next.push_back({f[0], a, c});
            next.push_back({f[1], b, a});
            next.push_back({f[2], c, b});
            next.push_back({a, b, c});
        }
        faces.swap(next);
    }
    std::vector<vec3> pos(verts.size()), nrm(verts.size());
    for (size_t i = 0; i < verts.size(); ++i) {
        nrm[i] = v3((float)verts[i][0], (float)verts[i][1], (float)verts[i][2]);
        pos[i] = centre + nrm[i] * radius;
    }
    for (const auto& f : faces)
        trianglesVec.push_back(Triangle(pos[(size_t)f[0]], pos[(size_t)f[1]], pos[(size_t)f[2]], nrm[(size_t)f[0]], nrm[(size_t)f[1]], nrm[(size_t)f[2]], materialIdx));
}
