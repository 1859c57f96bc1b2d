/* immesh_shade.h -- shaded and coloured images of the mesh on the device (libimmesh_hip.so).
 *
 * Reference: the GUI's main view.  draw_triangle draws the mesh through Triangle_facet_shader:
 *   src/meshing/mesh_rec_display.cpp:273-281                        draw_triangle
 *   src/meshing/mesh_rec_display.cpp:105-137, :264-265              the running axis range g_axis_min_max
 *   src/shader/tools_my_texture_triangle_shader.h:123-160           set_color_by_axis, set_pointcloud (one normal per facet, a packed 8-bit colour per vertex)
 *   src/shader/tools_my_texture_triangle_shader.h:164-208           draw
 *   src/shader/triangle_facets.vs / .fs                             smooth colour, two-sided Lambert light at the camera: 0.2 + 0.5 |n . l|
 *   src/tools/tinycolormap.hpp                                      GetHeatColor, CalcLerp, Clamp01
 * With per-vertex colours (include/immesh_colour.h) in place of the height map the same pass is README 2.3's texture view.  Here it is one more pass
 * behind the rasterizer of include/immesh_render.h: the winner face per pixel and the per-face records are already in HBM, the pass shades them.
 *
 * These declarations are part of the C ABI of immesh_c_api.h (which includes this file).  The checker is a restatement of the contract below
 * (tests/shade_checker.py, on top of tests/render_checker.py), not the oracle.
 *
 * ---- Contract (exact; all arithmetic in IEEE double, in the order written, no fused multiply-add, unless a line says float) -----------------
 *   A shade call is a render (include/immesh_render.h) plus a colour pass: depth_out / face_out are the render's, byte for byte;
 *   immesh_render_points and immesh_renderer_last_timing work after it exactly as after immesh_render_triangles / immesh_render_mesh.
 *   Vertex colour C (three bytes, in output order R, G, B):
 *     WHITE:   255, 255, 255.
 *     AXIS:    lo = (float)axis_min, hi = (float)axis_max after resolution (below).  In float, as set_color_by_axis:
 *              val = (p[axis] - lo) / (hi - lo);  hi <= lo: val = 0.  Then x = 1.0 - (double)val and Heat as tinycolormap's CalcLerp over
 *              T = (0,0,1), (0,1,1), (0,1,0), (1,1,0), (1,0,0):  m = x < 1.0 ? x : 1.0;  c = 0.0 < m ? m : 0.0  (Clamp01: std::min, std::max; a NaN
 *              gives 1);  a = c 4;  i = floor(a);  t = a - i;  col[k] = (1.0 - t) T[i][k] + t T[ceil(a)][k];  C[k] = (uint8)(col[k] 255), truncated.
 *              Resolution: axis_min >= axis_max asks for the range of the vertices: the minimum and maximum of coordinate `axis` over every vertex
 *              (of vtx_xyz, or of the export; referenced by a face or not) whose three coordinates are finite; with no such vertex 0 / 0.  The
 *              reference keeps a running range over everything ever displayed; a caller who wants that passes the range in.
 *     VERTEX:  the caller's bytes (immesh_shade_triangles), or what immesh_colour_fetch gives for the vertex (immesh_shade_mesh: export vertex i is
 *              vertex i of the map, as in immesh_save_ply_rgb), 0, 0, 0 when n_obs < min_views.  C = (m[0], m[1], m[2]) of the memory channels m;
 *              bgr = 1: C = (m[2], m[1], m[0]).  min_views is read with a colourer only.
 *   Pixel:   the winner face of the render contract with its e0, e1, e2, nd, n, dir at this pixel; a, b, c the face's vertices in index order.
 *              E = (e0 + e1) + e2;  wa = e1 / E, wb = e2 / E, wc = e0 / E  (bc . p = wa det for a point p of the plane: object-space weights, so the
 *              interpolation is perspective-correct, as GL's smooth varying);  E == 0: wa = wb = wc = 1.0 / 3.0 (keeps the function total).
 *              obj[k] = ((wa Ca[k] + wb Cb[k]) + wc Cc[k]) / 255.0.
 *              light == 0: L = 1.  Else L = 0.2 + (fabs(nd) / (sqrt(dot(n, n)) sqrt(dot(dir, dir)))) 0.5: the facet normal against the direction to the
 *              camera centre, both in the camera frame (the angle is rotation-invariant); sqrt correctly rounded.
 *              out[k] = (uint8)floor(fmin(fmax(L obj[k], 0), 1) 255 + 0.5)  (fmin / fmax: a NaN gives 0).
 *            A pixel without a face (face -1) gets `background`.  rgb_out is height x width x 3 bytes, row-major, row 0 at the top, R first.
 * Not reproduced: GL's float precision; GL's sampling at pixel centres (the render contract fixes the ray through the integer pixel); the wireframe
 * mode of m_if_draw_face == false (GL line rasterization has no exact restatement); blending and alpha.
 * Arguments are validated before any launch, after the camera's (immesh_render.h): a known source, 0 <= axis <= 2, axis_min and axis_max finite as
 * floats, VERTEX with colours (immesh_shade_triangles) or with a colourer of the renderer's context (immesh_shade_mesh); else IMMESH_E_INVAL with
 * text in immesh_last_error(ctx), nothing launched and no output written.  axis and the range are checked for every source.
 */
#ifndef IMMESH_SHADE_H
#define IMMESH_SHADE_H
#include "immesh_c_api.h"
#ifdef __cplusplus
extern "C" {
#endif

#define IMMESH_SHADE_WHITE  0   /* set_pointcloud without axis_min_max: 255,255,255 */
#define IMMESH_SHADE_AXIS   1   /* set_color_by_axis: Heat over one coordinate */
#define IMMESH_SHADE_VERTEX 2   /* per-vertex 8-bit colours */

typedef struct immesh_shade {
    int32_t source;        /* one of the above */
    int32_t axis;          /* 0..2; the reference uses 2 */
    int32_t light;         /* 1: the fragment shader's if_light branch; 0: objectColor as it is */
    int32_t bgr;           /* VERTEX: 1 takes red from memory channel 2 (as immesh_save_ply_rgb) */
    int32_t min_views;     /* VERTEX from a colourer: n_obs < min_views -> 0,0,0 (as immesh_save_ply_rgb) */
    uint8_t background[3]; /* pixels without a face */
    uint8_t pad;
    double  axis_min, axis_max;   /* AXIS: axis_min >= axis_max -> taken from the vertices */
} immesh_shade;

/* WHITE, axis 2, light 1, bgr 0, min_views 0, background 0, range 0 / 0 */
void immesh_default_shade(immesh_shade* sh);

/* immesh_render_triangles plus the colour pass.  vtx_rgb (n_vtx x 3 bytes, memory-channel order) is read for VERTEX only.  Any output may be NULL. */
int immesh_shade_triangles(immesh_renderer* r, const immesh_camera* cam, const float* vtx_xyz, int64_t n_vtx, const int32_t* faces, int64_t n_faces,
                           const uint8_t* vtx_rgb, const immesh_shade* sh, uint8_t* rgb_out, float* depth_out, int32_t* face_out);
/* immesh_render_mesh plus the colour pass, with its threading rule: call from the thread that drives the scan loop.  Drains queued mesh jobs; neither
 * the map nor the colourer's state is modified (the state is read where it lies in HBM).  colourer is read for VERTEX only and must belong to the
 * renderer's context.  A context with shard_mesh set returns IMMESH_E_INVAL, as the colourer's calls do. */
int immesh_shade_mesh(immesh_renderer* r, const immesh_camera* cam, immesh_colourer* colourer, double smooth_factor, int32_t knn, const immesh_shade* sh,
                      uint8_t* rgb_out, float* depth_out, int32_t* face_out);
/* lo, hi (the floats, widened) that the last successful shade call used; 0 / 0 when its source was not AXIS */
int immesh_shade_range(immesh_renderer* r, double lo_hi[2]);
/* Device time of the colour pass of the last shade call alone (range, vertex colours, pixels), milliseconds from HIP events on the renderer's stream;
 * the rasterize and reinforce times of the same call are immesh_renderer_last_timing's. */
int immesh_renderer_last_shade_ms(immesh_renderer* r, float* ms);

#ifdef __cplusplus
}
#endif
#endif
