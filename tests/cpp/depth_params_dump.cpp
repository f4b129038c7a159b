// depth_params_dump — TEST INFRASTRUCTURE: limo_amd/kba/depth_params_yaml.hpp over a zeroed limo_depth_params; prints the
// struct's bytes as hex (tests/test_depth_modes.py compares them with the Python reader's), or the error and exit code 2.
#include <cstdio>
#include <cstring>

#include "../../limo_amd/kba/depth_params_yaml.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 3;
    limo_depth_params p;
    std::memset(&p, 0, sizeof(p));
    std::string err;
    if (!keyframe_bundle_adjustment::depth_params_yaml::load(argv[1], &p, &err)) {
        std::fprintf(stderr, "%s\n", err.c_str());
        return 2;
    }
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&p);
    for (size_t k = 0; k < sizeof(p); ++k) std::printf("%02x", b[k]);
    std::printf("\n");
    return 0;
}
