// Host check of StepGraph's ownership paths (csrc/dstep.h) on objects that never captured: construction, move
// construction, move assignment (onto another object, onto itself, inside containers) and destruction must neither touch
// the HIP runtime with a handle they do not own nor leave one behind.  The capture itself needs a device and is covered by
// the GPU tests.  Stand-alone: build with the host sanitizers and run, from the repository root:
//   hipcc --offload-arch=gfx950 -std=c++17 -x hip -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tests/host/stepgraph_host.cpp seamless_communication_amd/csrc/common.cpp -o build/stepgraph_host && build/stepgraph_host
#include <cstdio>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../seamless_communication_amd/csrc/dstep.h"

namespace sc {
std::mutex& capture_mutex() {
    static std::mutex mu;
    return mu;
}
}  // namespace sc

int main() {
    using sc::StepGraph;
    static_assert(!std::is_copy_constructible<StepGraph>::value && !std::is_copy_assignable<StepGraph>::value, "StepGraph owns its pair");
    static_assert(std::is_nothrow_move_constructible<StepGraph>::value && std::is_nothrow_move_assignable<StepGraph>::value, "movable");
    int bad = 0;
    StepGraph a;
    bad += a.ready();
    StepGraph b(std::move(a));
    bad += a.ready() + b.ready();
    StepGraph c;
    c = std::move(b);
    StepGraph& self = c;
    c = std::move(self);
    bad += b.ready() + c.ready();
    StepGraph parity[2];  // the beam search's pair
    parity[0] = std::move(parity[1]);
    bad += parity[0].ready() + parity[1].ready();
    std::vector<StepGraph> v(3);
    for (int i = 0; i < 20; ++i) v.emplace_back();  // reallocation moves every element
    v.erase(v.begin());
    for (const StepGraph& g : v) bad += g.ready();
    struct Session {  // a member of an owner that is heap-allocated and dropped, as DecodeSession is
        StepGraph graph, cgraph;
    };
    std::unique_ptr<Session> s(new Session());
    std::unique_ptr<Session> t = std::move(s);
    t.reset();
    printf(bad ? "stepgraph_host: FAILED (%d)\n" : "stepgraph_host: ok\n", bad);
    return bad ? 1 : 0;
}
