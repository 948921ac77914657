// Prints project_camera and ray_camera of include/sadvio_cameras.hpp for a fixed table of points and pixels per model, so
// that tests/test_camera_models_cpu.py can hold the Python restatement (tests/camera_models.py) to this header. Host only.
//   M <model> <kind> fx fy cx cy width height rmax xi alpha distortion D0 D1 D2 D3
//   P <model> x y z u v verdict
//   R <model> u v rx ry rz
#include <cstdio>

#include "sadvio_cameras.hpp"

using namespace sadvio;

static CameraIntrinsics make(CameraKind kind, double fx, double fy, double cx, double cy, double rmax, double xi, double alpha, bool dist) {
    CameraIntrinsics c;
    c.kind = kind; c.fx = fx; c.fy = fy; c.cx = cx; c.cy = cy; c.width = 752; c.height = 480; c.rmax = rmax; c.xi = xi; c.alpha = alpha;
    c.distortion = dist;
    if (dist) { c.D[0] = -0.05; c.D[1] = 0.01; c.D[2] = 0.001; c.D[3] = -0.0005; }
    return c;
}

int main() {
    const CameraIntrinsics models[] = {
        make(CameraKind::Pinhole, 458.654, 457.296, 367.215, 248.375, 1, 0, 0, false),
        make(CameraKind::FisheyeEquidistant, 1.1, 1.1, 376.0, 240.0, 300.0, 0, 0, false),
        make(CameraKind::FisheyeEquisolid, 1.05, 1.05, 370.5, 236.0, 310.0, 0, 0, false),
        make(CameraKind::FisheyeStereographic, 0.95, 0.95, 380.25, 244.5, 290.0, 0, 0, false),
        make(CameraKind::Omni, 300.0, 301.0, 376.0, 240.0, 1, 0.3 / 0.7, 0.3, false),
        make(CameraKind::Omni, 305.0, 304.0, 372.0, 238.0, 1, 0.7 / 0.3, 0.7, true),
        make(CameraKind::Omni, 300.0, 300.0, 376.0, 240.0, 1, 1.0, 0.5, true),          // the xi == 1 lift
        make(CameraKind::DoubleSphere, 350.0, 352.0, 376.0, 240.0, 1, -0.2, 0.3, false),
        make(CameraKind::DoubleSphere, 348.0, 351.0, 371.0, 243.0, 1, 0.1, 0.7, false),
        make(CameraKind::DoubleSphere, 350.0, 352.0, 376.0, 240.0, 1, -0.2, 0.58, false),
    };
    // valid, near the axis, behind both depth limits, between them (z = 0.05), wide angle, far outside the image, behind the camera
    const double pts[][3] = {{0.4, -0.3, 4.0}, {-1.1, 0.6, 3.2}, {0.004, 0.003, 5.0}, {0.2, 0.1, 0.005}, {0.02, 0.01, 0.05}, {-0.09, 0.01, 0.05},
                             {2.5, 1.0, 1.2}, {40.0, 0.5, 4.0}, {0.3, 0.2, -2.0}, {0.0, 0.0, 3.0}, {1.0, -2.0, 0.1}, {0.7, 0.2, 0.0999}};
    const double pix[][2] = {{400.0, 260.0}, {120.5, 60.25}, {700.0, 430.0}, {376.5, 240.25}, {20.0, 470.0}};
    for (int m = 0; m < (int)(sizeof(models) / sizeof(models[0])); m++) {
        const CameraIntrinsics& c = models[m];
        std::printf("M %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %.17g %.17g %.17g %.17g\n", m, (int)c.kind, c.fx, c.fy, c.cx, c.cy,
                    c.width, c.height, c.rmax, c.xi, c.alpha, c.distortion ? 1 : 0, c.D[0], c.D[1], c.D[2], c.D[3]);
        for (const auto& p : pts) {
            double u = 0, v = 0;
            const bool ok = project_camera(c, p, u, v);
            std::printf("P %d %.17g %.17g %.17g %.17g %.17g %d\n", m, p[0], p[1], p[2], u, v, ok ? 1 : 0);
        }
        for (const auto& q : pix) {
            double r[3] = {0, 0, 0};
            ray_camera(c, q[0], q[1], r);
            std::printf("R %d %.17g %.17g %.17g %.17g %.17g\n", m, q[0], q[1], r[0], r[1], r[2]);
        }
    }
    return 0;
}
