// tests/golden/volume_ref.cpp -- fixture generator for the volume support (vrh_render_volume, vrh_tex3d_host,
// vrh_tex1d_host).
//
// Runs the reference's own tex3D / tex1D and the loop of its volume example (src/examples/volume/main.cpp:
// 123-167) with scalar float rays on the CPU, from the reference's headers (never copied into this
// repository), over a file written by make_volume_golden.py:
//
//     volume_ref <in.bin> <out.bin>
//
// in.bin starts with a u32 magic 0x564F4C52 and a u32 mode.  Texel storage is guarded as in
// textured_ref.cpp: the arrays lie between runs of guard texels (guard 0: zeros; guard 1: the largest
// value of the format, 3e38 for floats), the script runs everything with both, and whatever differs read
// outside its array (the reference reads texel N of an axis for a Wrap coordinate that maps to exactly 1.0).
//
// mode 0, tex3D samples: u32 W, H, D, format (0 unorm<8>, 1 unorm<16>, 2 float), filter, address x, y, z, n,
// guard; the voxels; n coordinate triples.  out.bin: n floats.
// mode 1, tex1D samples: u32 N, filter, address, n, guard; N x 4 floats; n coordinates.  out.bin: n x 4 floats.
// mode 2, frame: the `frame_header` below, the voxels, the transfer function.  out.bin: per pixel the
// colour (4 floats), then per pixel hit (u32), tnear (float), steps (u32), then the u64 total of the steps.
// With `example` set the loop is the example's text verbatim (its texture coordinate expressions, its
// 0.01f step, its double 0.999); otherwise the generalised form tc = (sign * pos + offset) / extent and a
// double cutoff.
#include <visionaray/math/math.h>
#include <visionaray/texture/texture.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace visionaray;

struct frame_header
{
    uint32_t W, H;
    uint32_t vw, vh, vd, format, filter, address[3];
    uint32_t tf_size, tf_filter, tf_address;
    uint32_t guard, example, pad;
    float box_min[3], box_max[3], sign[3], offset[3], extent[3];
    float dt;
    double cutoff;
    float eye[3], cam_u[3], cam_v[3], cam_w[3];
};

template <typename T> struct guard_value;
template <> struct guard_value<uint8_t> { static uint8_t get(uint32_t g) { return g ? 255 : 0; } };
template <> struct guard_value<uint16_t> { static uint16_t get(uint32_t g) { return g ? 65535 : 0; } };
template <> struct guard_value<float> { static float get(uint32_t g) { return g ? 3.0e38f : 0.0f; } };

// n texels of S between two runs of `pad` guard texels
template <typename S>
struct guarded
{
    std::vector<S> store;
    size_t pad = 0;
    bool read(FILE* in, size_t n, size_t pad_, uint32_t guard)
    {
        pad = pad_;
        store.assign(2 * pad + n, guard_value<S>::get(guard));
        return fread(store.data() + pad, sizeof(S), n, in) == n;
    }
    const S* data() const { return store.data() + pad; }
};

struct guarded_tf
{
    std::vector<float> store;
    bool read(FILE* in, size_t n, uint32_t guard)
    {
        store.assign((n + 16) * 4, guard_value<float>::get(guard));
        return fread(store.data() + 32, 16, n, in) == n;
    }
    texture_ref<vec4, 1> ref(uint32_t n, uint32_t filter, uint32_t address) const
    {
        texture_ref<vec4, 1> t(n);
        t.reset(reinterpret_cast<vec4 const*>(store.data() + 32));
        t.set_filter_mode(filter == 0 ? Nearest : Linear);
        t.set_address_mode(tex_address_mode(address));
        return t;
    }
};

template <typename T>
static texture_ref<T, 3> volume_ref(const void* data, const uint32_t dims[3], uint32_t filter, const uint32_t address[3])
{
    texture_ref<T, 3> t(dims[0], dims[1], dims[2]);
    t.reset(reinterpret_cast<T const*>(data));
    t.set_filter_mode(filter == 0 ? Nearest : Linear);
    for (int a = 0; a < 3; ++a) t.set_address_mode(a, tex_address_mode(address[a]));
    return t;
}

static size_t volume_pad(const uint32_t dims[3]) { return 2 * size_t(dims[0]) * dims[1] + 2 * size_t(dims[0]) + 8; }

template <typename T, typename S>
static int samples3d(FILE* in, FILE* out, const uint32_t* d)
{
    const uint32_t dims[3] = { d[0], d[1], d[2] }, address[3] = { d[5], d[6], d[7] }, n = d[8];
    guarded<S> g;
    if (!g.read(in, size_t(dims[0]) * dims[1] * dims[2], volume_pad(dims), d[9])) return 3;
    std::vector<float> coords(size_t(n) * 3), res(n);
    if (fread(coords.data(), 12, n, in) != n) return 3;
    auto t = volume_ref<T>(g.data(), dims, d[4], address);
    for (uint32_t i = 0; i < n; ++i) res[i] = tex3D(t, vec3(coords[3 * i], coords[3 * i + 1], coords[3 * i + 2]));
    return fwrite(res.data(), 4, n, out) == n ? 0 : 4;
}

static int samples1d(FILE* in, FILE* out)
{
    uint32_t d[5];
    if (fread(d, 4, 5, in) != 5) return 3;
    guarded_tf g;
    if (!g.read(in, d[0], d[4])) return 3;
    const uint32_t n = d[3];
    std::vector<float> coords(n), res(size_t(n) * 4);
    if (n && fread(coords.data(), 4, n, in) != n) return 3;
    auto t = g.ref(d[0], d[1], d[2]);
    for (uint32_t i = 0; i < n; ++i)
    {
        vec4 c = tex1D(t, coords[i]);
        res[4 * i] = c.x; res[4 * i + 1] = c.y; res[4 * i + 2] = c.z; res[4 * i + 3] = c.w;
    }
    return fwrite(res.data(), 16, n, out) == n ? 0 : 4;
}

template <typename T, typename S>
static int frame(FILE* in, FILE* out, const frame_header& h)
{
    const uint32_t dims[3] = { h.vw, h.vh, h.vd };
    guarded<S> g;
    if (!g.read(in, size_t(dims[0]) * dims[1] * dims[2], volume_pad(dims), h.guard)) return 3;
    guarded_tf gt;
    if (!gt.read(in, h.tf_size, h.guard)) return 3;
    auto volume = volume_ref<T>(g.data(), dims, h.filter, h.address);
    auto transfunc = gt.ref(h.tf_size, h.tf_filter, h.tf_address);
    const aabb bbox(vec3(h.box_min[0], h.box_min[1], h.box_min[2]), vec3(h.box_max[0], h.box_max[1], h.box_max[2]));
    const vec3 eye(h.eye[0], h.eye[1], h.eye[2]), cam_u(h.cam_u[0], h.cam_u[1], h.cam_u[2]);
    const vec3 cam_v(h.cam_v[0], h.cam_v[1], h.cam_v[2]), cam_w(h.cam_w[0], h.cam_w[1], h.cam_w[2]);
    const size_t npx = size_t(h.W) * h.H;
    std::vector<float> color(npx * 4), tnear(npx);
    std::vector<uint32_t> hit(npx), steps(npx);
    uint64_t total = 0;
    for (uint32_t y = 0; y < h.H; ++y)
        for (uint32_t x = 0; x < h.W; ++x)
        {
            // the primary ray of the pinhole camera (sched_common.h:130-150), uniform pixel sampler
            const float u = 2.0f * (float(x) + 0.5f) / float(h.W) - 1.0f;
            const float v = 2.0f * (float(y) + 0.5f) / float(h.H) - 1.0f;
            basic_ray<float> ray;
            ray.ori = eye;
            ray.dir = normalize(cam_u * u + cam_v * v + cam_w);

            auto hit_rec = intersect(ray, bbox);
            auto t = hit_rec.tnear;
            vec4 result(0.0f);
            uint32_t n = 0;
            while (t < hit_rec.tfar)
            {
                ++n;
                auto pos = ray.ori + ray.dir * t;
                vec3 tex_coord;
                if (h.example)
                    tex_coord = vec3(( pos.x + 1.0f ) / 2.0f, (-pos.y + 1.0f ) / 2.0f, (-pos.z + 1.0f ) / 2.0f);
                else
                    tex_coord = vec3((h.sign[0] * pos.x + h.offset[0]) / h.extent[0], (h.sign[1] * pos.y + h.offset[1]) / h.extent[1],
                                     (h.sign[2] * pos.z + h.offset[2]) / h.extent[2]);
                auto voxel = tex3D(volume, tex_coord);
                vec4 c = tex1D(transfunc, voxel);
                c.xyz() *= c.w;
                result += c * (1.0f - result.w);
                if (h.example ? result.w >= 0.999 : result.w >= h.cutoff) break;
                if (h.example) t += 0.01f;
                else t += h.dt;
            }
            const size_t o = size_t(y) * h.W + x;
            color[4 * o] = result.x; color[4 * o + 1] = result.y; color[4 * o + 2] = result.z; color[4 * o + 3] = result.w;
            hit[o] = hit_rec.hit ? 1u : 0u;
            tnear[o] = hit_rec.tnear;
            steps[o] = n;
            total += n;
        }
    if (fwrite(color.data(), 16, npx, out) != npx || fwrite(hit.data(), 4, npx, out) != npx
        || fwrite(tnear.data(), 4, npx, out) != npx || fwrite(steps.data(), 4, npx, out) != npx || fwrite(&total, 8, 1, out) != 1)
        return 4;
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: volume_ref <in.bin> <out.bin>\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint32_t head[2];
    if (fread(head, 4, 2, in) != 2 || head[0] != 0x564F4C52u) return 3;
    int rc = 3;
    if (head[1] == 0)
    {
        uint32_t d[10];
        if (fread(d, 4, 10, in) == 10)
            rc = d[3] == 0 ? samples3d<unorm<8>, uint8_t>(in, out, d)
               : d[3] == 1 ? samples3d<unorm<16>, uint16_t>(in, out, d) : samples3d<float, float>(in, out, d);
    }
    else if (head[1] == 1) rc = samples1d(in, out);
    else if (head[1] == 2)
    {
        frame_header h;
        if (fread(&h, sizeof(h), 1, in) == 1)
            rc = h.format == 0 ? frame<unorm<8>, uint8_t>(in, out, h)
               : h.format == 1 ? frame<unorm<16>, uint16_t>(in, out, h) : frame<float, float>(in, out, h);
    }
    fclose(in);
    fclose(out);
    return rc;
}
