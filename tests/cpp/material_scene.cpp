// material_scene.cpp — materials through the C++ host mirror (include/physics_state.hpp): RigidBody::friction /
// restitution as pub fields and PhysicsState::set_ground_material. A ball dropped on the ground and a ball sliding on
// it; the materials are edited between frames, taken back to the defaults, and reset by a body edit. Prints the final
// state as JSON; tests/test_gpu_material_mirror.py replays the same sequence of C ABI calls on a World.
#include <cstdio>

#include "physics_state.hpp"

using namespace physics;

int main() {
    try {
        phys_config cfg;
        phys_config_default(&cfg);
        cfg.flags = PHYS_FLAG_COLLISIONS | PHYS_FLAG_GROUND_PLANE;
        cfg.gravity_offset[0] = 0.0f; cfg.gravity_offset[1] = 0.0f; cfg.gravity_offset[2] = 0.0f;
        PhysicsState state(&cfg);
        for (size_t i = 0; i < 2; ++i) {
            rigid_body::RigidBody b = rigid_body::RigidBody::new_(i);
            b.shape_type = PHYS_SHAPE_SPHERE;
            b.half_extent = Vector3(0.5f, 0.5f, 0.5f);
            state.entities.push_back(Entity{b, 0});
        }
        state.entities[0].body.position = Vector3(0.0f, 1.3f, 0.0f);
        state.entities[0].body.restitution = 0.8f;
        state.entities[1].body.position = Vector3(4.0f, 0.5f, 0.0f);
        state.entities[1].body.lin_velocity = Vector3(3.0f, 0.0f, 0.0f);
        state.entities[1].body.friction = 0.1f;
        state.set_ground_material(0.4f, 0.0f);
        const Duration dt(16666667);
        for (int f = 0; f < 40; ++f) {
            if (f == 20) state.entities[1].body.friction = 0.9f;  // a material edit alone
            if (f == 30)                                          // back to the defaults: the upload is taken back
                for (auto& e : state.entities) { e.body.friction = -1.0f; e.body.restitution = 0.0f; }
            if (f == 35) state.entities[0].body.position.x = 1.0f;  // a body edit: phys_set_bodies resets the materials
            state.update(dt);
        }
        std::printf("{\"pos\": [");
        for (size_t i = 0; i < 2; ++i) {
            const auto& b = state.entities[i].body;
            std::printf("%s[%.9g, %.9g, %.9g]", i ? ", " : "", b.position.x, b.position.y, b.position.z);
        }
        std::printf("], \"lin\": [");
        for (size_t i = 0; i < 2; ++i) {
            const auto& b = state.entities[i].body;
            std::printf("%s[%.9g, %.9g, %.9g]", i ? ", " : "", b.lin_velocity.x, b.lin_velocity.y, b.lin_velocity.z);
        }
        std::printf("]}\n");
    } catch (const Panic& p) {
        std::fprintf(stderr, "panic %d: %s\n", p.code, p.what());
        return 1;
    }
    return 0;
}
