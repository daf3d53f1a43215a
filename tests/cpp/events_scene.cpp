// events_scene — contact events through the C++ host mirror (include/physics_state.hpp): a few spheres and a box dropped
// onto the ground and onto each other, one more hopping off the ground, 90 updates, one drain. Prints the drained events as hex bytes and the impulse
// rows of the last update; tests/test_gpu_events_mirror.py runs the same scene on a Python World and compares the bytes.
#include <cstdio>

#include "physics_state.hpp"

int main() {
    using namespace physics;
    phys_config cfg;
    phys_config_default(&cfg);
    cfg.flags = PHYS_FLAG_COLLISIONS | PHYS_FLAG_GROUND_PLANE;
    cfg.gravity_offset[0] = cfg.gravity_offset[1] = cfg.gravity_offset[2] = 0.0f;
    try {
        PhysicsState ps(&cfg);
        const float at[5][3] = {{0.0f, 0.8f, 0.0f}, {0.1f, 2.1f, 0.0f}, {3.0f, 1.5f, 0.0f}, {3.2f, 3.0f, 0.1f}, {-4.0f, 0.5f, 2.0f}};
        for (size_t i = 0; i < 5; ++i) {
            Entity e;
            e.body = rigid_body::RigidBody::new_(i);
            e.body.position = Vector3(at[i][0], at[i][1], at[i][2]);
            e.body.shape_type = i == 2 ? PHYS_SHAPE_BOX : PHYS_SHAPE_SPHERE;
            e.body.half_extent = Vector3(0.5f, 0.5f, 0.5f);
            if (i == 4) e.body.lin_velocity = Vector3(0.0f, 3.0f, 0.0f);  // touches the ground, leaves it, comes back
            ps.entities.push_back(e);
        }
        ps.enable_contact_events(4096);
        for (int f = 0; f < 90; ++f) ps.update(Duration(16666667));
        uint64_t dropped = 0;
        const std::vector<PhysicsState::ContactEvent> ev = ps.drain_contact_events(&dropped);
        const auto imp = ps.contact_impulses();
        std::printf("{\"dropped\": %llu, \"n\": %zu, \"events\": \"", (unsigned long long)dropped, ev.size());
        const unsigned char* b = reinterpret_cast<const unsigned char*>(ev.data());
        for (size_t k = 0; k < ev.size() * sizeof(PhysicsState::ContactEvent); ++k) std::printf("%02x", b[k]);
        std::printf("\", \"impulses\": \"");
        b = reinterpret_cast<const unsigned char*>(imp.data());
        for (size_t k = 0; k < imp.size() * 48; ++k) std::printf("%02x", b[k]);
        std::printf("\", \"after\": %zu}\n", ps.drain_contact_events().size());
    } catch (const Panic& p) {
        std::fprintf(stderr, "panic %d: %s\n", p.code, p.what());
        return 1;
    }
    return 0;
}
