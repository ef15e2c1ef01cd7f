// Kernel instantiations of the CRT-encryption Garner lift (kernels_crt_lift.hpp): the lane-group geometries that hold the
// q^2 of the keys the route serves (primes of 700 .. 1024 and 1400 .. 2068 bits: 72, 112 and 144 limbs).
#include "geo_ops.hpp"
#include "kernels_crt_lift.hpp"
#include "launch.hpp"

namespace pai {

namespace {
template <class G>
struct LiftLaunch {
    static void lift(hipStream_t s, int grid, const CrtLiftParams& P, const uint32_t* c_in, uint32_t* ct_out, int n) {
        launch(k_crt_lift<G>, dim3(grid), dim3(BLOCK_THREADS), 2 * G::LDS_WORDS * 4, s, P, c_in, ct_out, n);
    }
    static CrtLiftOps ops() {
        CrtLiftOps t{};
        t.nl = G::NL;
        t.epb = G::EPB;
        t.lift = &lift;
        return t;
    }
};
}  // namespace

const CrtLiftOps* crt_lift_ops(int nl) {
    static const CrtLiftOps o72 = LiftLaunch<Geo<36, 2, 6, false>>::ops();
    static const CrtLiftOps o112 = LiftLaunch<Geo<28, 4, 4, false>>::ops();
    static const CrtLiftOps o144 = LiftLaunch<Geo<36, 4, 6, false>>::ops();
    return nl == 72 ? &o72 : (nl == 112 ? &o112 : (nl == 144 ? &o144 : nullptr));
}

}  // namespace pai
