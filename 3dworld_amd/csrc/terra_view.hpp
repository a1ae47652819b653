// terra_view.hpp -- the view frustum and the box primitives every camera pass shares: pos_dir_up (src/visibility.cpp:67-103,119-128,141-174,186-196,215-219;
// cube_visible_likely, src/3DWorld.h:724) with cube_t::closest_pt / closest_pt_dist_sq / closest_dist_less_than (src/3DWorld.h:591,636-641; src/csg.cpp:244-247),
// dist_less_than (src/inlines.h:176-192), orthogonalize_dir (:265-268), InvSqrt (:39-50) and cube_t::union_with_cube / assign_or_union_with_cube
// (src/3DWorld.h:506-527).  The line clip and the x86 conversions are terra_common.hpp's.
//
// These are the leaves that tests/golden/primitive_vectors.npz pins to the reference's compiled code, on the host and on gfx950 (tests/devprobe): a pass calls
// them from here and keeps no copy.  Every operand carries the type the reference statement gives it; where the C++ source promotes to double the promotion is
// written out; dot products are summed in the reference's order (the library is built without contraction).
//
// The tests are pure: where the reference leaves a loop early (check_clip_plane's first passing point, the near / far loop of pt_set_visible) the bodies here
// evaluate every term and combine them -- the same booleans, no branch per term.
#pragma once
#include "terra_common.hpp"

namespace terra {

struct view_pod_t {float pos[3], dir[3], upv[3], cp[3]; float sterm, x_sterm, near_, far_; int32_t valid;}; // terra_view: pos_dir_up's pos, dir, upv_, cp, ...

// ---- pos_dir_up's constructor (:67-85) and orthogonalize_up_dir (:87-92) with the C library's tanf / sinf / atanf.  false where the constructor asserts.
inline bool view_make(float const pos[3], float const dir[3], float const up[3], float angle, float aspect, float near_, float far_, view_pod_t &o) {
	if (!(near_ >= 0.0f && far_ > 0.0f && far_ > near_)) return false;
	if (dir[0] == 0.0f && dir[1] == 0.0f && dir[2] == 0.0f) return false; // assert(dir != zero_vector)
	double const A = (double)aspect;
	float const tterm = tanf(angle), sterm = sinf(angle);
	float x_sterm;
	if (A == 1.0) {x_sterm = sterm;}
	else {
		if (!(tterm > 0.0f)) return false; // angle < 90
		float atan_val = atanf((float)(A*(double)tterm));
		if (atan_val < 0.0f) {atan_val += PI_F;}
		x_sterm = (atan_val/angle)*sterm;
	}
	for (int k = 0; k < 3; ++k) {o.pos[k] = pos[k]; o.dir[k] = dir[k];}
	// orthogonalize_dir(upv, dir, upv_, 1): cross_product(dir, cross_product(upv, dir)), normalized (pointT::normalize, src/3DWorld.h:273-279)
	float const tx = up[1]*dir[2] - up[2]*dir[1], ty = up[2]*dir[0] - up[0]*dir[2], tz = up[0]*dir[1] - up[1]*dir[0];
	float ux = dir[1]*tz - dir[2]*ty, uy = dir[2]*tx - dir[0]*tz, uz = dir[0]*ty - dir[1]*tx;
	float const mag = sqrtf(ux*ux + uy*uy + uz*uz);
	if (mag >= 1.0E-12f) {float const m = (float)(1.0/(double)mag); ux *= m; uy *= m; uz *= m;}
	o.upv[0] = ux; o.upv[1] = uy; o.upv[2] = uz;
	o.cp[0] = dir[1]*uz - dir[2]*uy; o.cp[1] = dir[2]*ux - dir[0]*uz; o.cp[2] = dir[0]*uy - dir[1]*ux; // cross_product(dir, upv_, cp)
	o.sterm = sterm; o.x_sterm = x_sterm; o.near_ = near_; o.far_ = far_; o.valid = 1;
	return true;
}
// behind_sphere_mult = max(1.0, A*A)*max(1.0, 2.0f/((double)tterm*tterm*(1.0 + A*A))) (src/visibility.cpp:83): A is a double member, tterm the float tanf(angle)
inline float view_behind_sphere_mult(float angle, float aspect) {
	double const A = (double)aspect;
	float const tterm = tanf(angle);
	double const a = (1.0 < A*A) ? A*A : 1.0, q = (double)2.0f/(((double)tterm*(double)tterm)*(1.0 + A*A)), b = (1.0 < q) ? q : 1.0; // std::max(a, b) = (a < b) ? b : a
	return (float)(a*b);
}
TERRA_HD bool view_finite(view_pod_t const &v) {
	bool ok = isfinite(v.sterm) && isfinite(v.x_sterm) && isfinite(v.near_) && isfinite(v.far_);
	for (int k = 0; k < 3; ++k) {ok = ok && isfinite(v.pos[k]) && isfinite(v.dir[k]) && isfinite(v.upv[k]) && isfinite(v.cp[k]);}
	return ok;
}

TERRA_HD float view_dot(float const a[3], float x, float y, float z) {return a[0]*x + a[1]*y + a[2]*z;} // dot_product (src/inlines.h:220-222)

// pos_dir_up::point_visible_test (src/visibility.cpp:94-103)
TERRA_HD bool view_point_visible(view_pod_t const &v, float px, float py, float pz) {
	if (!v.valid) return true;
	float const x = px - v.pos[0], y = py - v.pos[1], z = pz - v.pos[2]; // vector3d const pv(pos_, pos)
	if (view_dot(v.dir, x, y, z) < 0.0f) return false;
	float const dist = sqrtf(x*x + y*y + z*z);
	if (fabsf(view_dot(v.upv, x, y, z)) > dist*v.sterm) return false;
	if (fabsf(view_dot(v.cp, x, y, z)) > dist*v.x_sterm) return false;
	return dist > v.near_ && dist < v.far_;
}
// pos_dir_up::sphere_visible_test (:119-128)
TERRA_HD bool view_sphere_visible(view_pod_t const &v, float behind_sphere_mult, float px, float py, float pz, float radius) {
	if (!v.valid) return radius >= 0.0f;
	float const x = px - v.pos[0], y = py - v.pos[1], z = pz - v.pos[2]; // vector3d const pv(pos_, pos)
	float const msq = x*x + y*y + z*z;
	if (view_dot(v.dir, x, y, z) < 0.0f) return radius > 0.0f && msq < radius*radius*behind_sphere_mult; // sphere behind
	float const dist = sqrtf(msq);
	if (fabsf(view_dot(v.upv, x, y, z)) > dist*v.sterm + radius) return false;
	if (fabsf(view_dot(v.cp, x, y, z)) > dist*v.x_sterm + radius) return false;
	return (dist + radius) > v.near_ && (dist - radius) < v.far_;
}
// pos_dir_up::cube_completely_visible (:186-196)
TERRA_HD bool view_cube_completely_visible(view_pod_t const &v, float const d[3][2]) {
	if (!v.valid) return true;
	bool all = true;
	for (int k = 0; k < 8; ++k) {all = all && view_point_visible(v, d[0][k >> 2], d[1][(k >> 1) & 1], d[2][k & 1]);}
	return all;
}
// cube_t::closest_pt_dist_sq(pos) = p2p_dist_sq(closest_pt(pos), pos), clamp_pt's min(d[1], max(d[0], p))
TERRA_HD float view_closest_dist_sq(float const d[3][2], float px, float py, float pz) {
	float const cx = min_std(d[0][1], max_std(d[0][0], px)), cy = min_std(d[1][1], max_std(d[1][0], py)), cz = min_std(d[2][1], max_std(d[2][0], pz));
	return (cx - px)*(cx - px) + (cy - py)*(cy - py) + (cz - pz)*(cz - pz);
}
// cube_t::closest_dist_less_than(pos, dist) = dist_less_than(pos, closest_pt(pos), dist)
TERRA_HD bool view_closest_dist_less_than(float const d[3][2], float px, float py, float pz, float dist) {return view_closest_dist_sq(d, px, py, pz) < dist*dist;}
// pos_dir_up::cube_visible (:165-174) with pt_set_visible<8> and check_clip_plane<8> (:141-163)
TERRA_HD bool view_cube_visible(view_pod_t const &v, float const d[3][2]) {
	if (!v.valid) return true;
	float const aau = v.sterm*v.sterm, aac = v.x_sterm*v.x_sterm;
	bool u0 = false, u1 = false, c0 = false, c1 = false, npass = false, fpass = false;
	for (int k = 0; k < 8; ++k) {
		float const x = d[0][k >> 2] - v.pos[0], y = d[1][(k >> 1) & 1] - v.pos[1], z = d[2][k & 1] - v.pos[2];
		float const msq = x*x + y*y + z*z, du = view_dot(v.upv, x, y, z), dc = view_dot(v.cp, x, y, z), dd = view_dot(v.dir, x, y, z);
		bool const iu = du*du <= aau*msq, ic = dc*dc <= aac*msq;
		u0 = u0 || du <= 0.0f || iu; u1 = u1 || -du <= 0.0f || iu; // (d ? -dp : dp) <= 0.0 || dp*dp <= aa*pv.mag_sq()
		c0 = c0 || dc <= 0.0f || ic; c1 = c1 || -dc <= 0.0f || ic;
		npass = npass || dd > v.near_; fpass = fpass || dd < v.far_;
	}
	if (!(u0 && u1 && c0 && c1 && npass && fpass)) return false;
	return view_closest_dist_less_than(d, v.pos[0], v.pos[1], v.pos[2], v.far_); // dist_less_than(pos, c.closest_pt(pos), far_)
}
// pos_dir_up::cube_visible_likely (src/3DWorld.h:724): the centre first, then the cube
TERRA_HD bool view_cube_visible_likely(view_pod_t const &v, float const d[3][2]) {
	if (!v.valid) return true;
	if (view_point_visible(v, 0.5f*(d[0][0] + d[0][1]), 0.5f*(d[1][0] + d[1][1]), 0.5f*(d[2][0] + d[2][1]))) return true; // get_cube_center()
	return view_cube_visible(v, d);
}
// pos_dir_up::sphere_and_cube_visible_test (src/visibility.cpp:215-219)
TERRA_HD bool view_sphere_and_cube_visible(view_pod_t const &v, float behind_sphere_mult, float cx, float cy, float cz, float r, float const d[3][2]) {
	if (!view_sphere_visible(v, behind_sphere_mult, cx, cy, cz, r)) return false; // none of the sphere is visible
	if (view_sphere_visible(v, behind_sphere_mult, cx, cy, cz, -r)) return true;  // all of the sphere is visible
	return view_cube_visible(v, d);
}

// InvSqrt (src/inlines.h:39-50): the bit trick with one iteration
TERRA_HD float inv_sqrt_ref(float x) {
	int32_t i; memcpy(&i, &x, 4);
	i = (int32_t)(0x5f3759dfu - (uint32_t)(i >> 1));
	float y; memcpy(&y, &i, 4);
	return y*(1.5f - 0.5f*x*y*y);
}

// ---- a box as six floats (x1, x2, y1, y2, z1, z2): cube_t::is_all_zeros, union_with_cube and assign_or_union_with_cube (src/3DWorld.h:491,506-527)
TERRA_HD bool box_all_zeros(float const d[6]) {return d[0] == 0.0f && d[1] == 0.0f && d[2] == 0.0f && d[3] == 0.0f && d[4] == 0.0f && d[5] == 0.0f;}
TERRA_HD void box_union(float bc[6], float const d[6]) {
	for (int k = 0; k < 6; k += 2) {bc[k] = min_std(bc[k], d[k]); bc[k + 1] = max_std(bc[k + 1], d[k + 1]);}
}
// a d of all zeros is ignored, a bc of all zeros is replaced
TERRA_HD void box_assign_or_union(float bc[6], float const d[6]) {
	if (!box_all_zeros(d)) {
		if (box_all_zeros(bc)) {for (int k = 0; k < 6; ++k) {bc[k] = d[k];}}
		else {box_union(bc, d);}
	}
}

// ---- the (key, index) order of the tree and deciduous draw lists and of the kernels' ranks: std::pair<float, unsigned>'s operator< and tree_inst_t's with the
// record index behind the id
TERRA_HD bool tree_view_before_f(float da, uint32_t ia, float db, uint32_t ib) {return da < db || (!(db < da) && ia < ib);}
TERRA_HD bool tree_view_before_u(uint32_t da, uint32_t ia, uint32_t db, uint32_t ib) {return da < db || (da == db && ia < ib);}

} // namespace terra
