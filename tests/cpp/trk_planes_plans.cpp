// The host-only plans of the plane ring and of tracking on planes through the C++ mirror (gnss-sdr-rs_amd/host/gnss_sdr.hpp):
// gnss::PlaneRing::plan and gnss::TrackingManager::planes_plan.  No device is needed.  tests/test_trk_planes_host.py writes the cases,
// one a line, and compares the lines printed here word for word with what the Python layer gives for the same cases:
//
//   ring <n_planes> <plane_size>
//   trk <fs> <n_channels> <n_arms> <code_len> <code_rate> <strict_sum_order> <n_planes> <max_epochs> <m0,m1,...|->
//
// code_len 0: the built-in C/A table; code_rate 0: the default; "-": no map (every channel on plane 0).  A refusal prints its status.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "gnss_sdr.hpp"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: trk_planes_plans <case file>\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string kind;
        if (!(s >> kind)) continue;
        try {
            if (kind == "ring") {
                uint32_t n_planes = 0; uint64_t plane_size = 0;
                s >> n_planes >> plane_size;
                const uint64_t bytes = gnss::PlaneRing::plan(n_planes, plane_size);
                std::cout << "ring bytes " << bytes << "\n";
            } else if (kind == "trk") {
                gm_trk_cfg c{};
                uint32_t code_len = 0, n_planes = 0, max_epochs = 0; int strict = 0;
                std::string map;
                s >> c.fs >> c.n_channels >> c.n_arms >> code_len >> c.nominal_code_rate >> strict >> n_planes >> max_epochs >> map;
                c.strict_sum_order = strict;
                std::vector<int8_t> chips(code_len ? code_len : 1, 1);
                if (code_len) { c.codes = chips.data(); c.n_codes = 1; c.code_len = code_len; }
                std::vector<uint32_t> planes;
                if (map != "-") {
                    std::istringstream m(map);
                    std::string w;
                    while (std::getline(m, w, ',')) planes.push_back(uint32_t(std::stoul(w)));
                }
                const gm_trk_planes_plan_out p = gnss::TrackingManager::planes_plan(c, n_planes, planes, max_epochs);
                std::cout << "trk workgroups " << p.workgroups << " threads " << p.threads << " chip_row_bytes " << p.chip_row_bytes << " planes_used "
                          << p.planes_used << " samples " << p.samples << " samples_per_lane " << p.samples_per_lane << " result_bytes "
                          << p.result_bytes << "\n";
            } else {
                std::cout << "unknown " << kind << "\n";
            }
        } catch (const gnss::Panic& e) {
            std::cout << kind << " refused " << e.status << "\n";
        }
    }
    return 0;
}
