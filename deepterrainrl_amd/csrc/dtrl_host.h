// dtrl_host.h -- host-side data layer of the engine: reference-format argument files, JSON data files, flattening of the
// character / controller / terrain descriptions into the POD tables the kernels read, and the per-env heightfield windows.
//
// Mirrors the reference's interfaces for this path (names and argument meaning kept):
//   cArgParser                 util/ArgParser.h:6-34, util/ArgParser.cpp:42-334
//   cKinTree::Load / LoadBodyDefs, cPDController::LoadParams, cDogController::LoadControllers / ReadParams
//   cTerrainGen2D (terrain functions + params), cGroundVar2D (two sliding segments)
#pragma once
#include "dtrl_types.h"
#include <map>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <vector>

namespace dtrl {

// ---- minimal JSON value (the data files are plain JSON; jsoncpp is not available in this image) ----
struct Json {
	enum Type { kNull, kBool, kNum, kStr, kArr, kObj } type = kNull;
	double num = 0; bool b = false; std::string str;
	std::vector<Json> arr;
	std::vector<std::pair<std::string, Json>> obj;
	const Json* find(const std::string& key) const;
	bool has(const std::string& key) const { const Json* j = find(key); return j && j->type != kNull; }
	double get_num(const std::string& key, double dflt) const { const Json* j = find(key); return (j && (j->type == kNum)) ? j->num : ((j && j->type == kBool) ? (j->b ? 1.0 : 0.0) : dflt); }
	bool get_bool(const std::string& key, bool dflt) const { const Json* j = find(key); if (!j) return dflt; if (j->type == kBool) return j->b; if (j->type == kNum) return j->num != 0; return dflt; }
	static bool parse(const std::string& text, Json& out, std::string& err);
	static bool parse_file(const std::string& path, Json& out, std::string& err);
};

// ---- cArgParser ----
class ArgParser {
public:
	ArgParser() {}
	ArgParser(const char* const* args, int n) { AppendArgs(args, n); }
	void AppendArgs(const char* const* args, int n);
	bool AppendArgs(const std::string& file);   // util/ArgParser.cpp:42-108
	bool ParseString(const std::string& key, std::string& out) const;
	bool ParseInt(const std::string& key, int& out) const;
	bool ParseDouble(const std::string& key, double& out) const;
	bool ParseBool(const std::string& key, bool& out) const;
	int GetNumArgs() const { return static_cast<int>(mArgs.size()); }
private:
	std::vector<std::string> mArgs;
	static bool IsKey(const std::string& s);
	int FindKeyIndex(const std::string& key) const;
};

// ---- terrain ----
// cRand restated over libstdc++ <random> (util/Rand.cpp): identical streams to the reference on the same libstdc++.
class TerrainRand {
public:
	void Seed(unsigned long s) { gen_.seed(s); }
	double RandDouble(double mn, double mx) { if (mn == mx) return mn; double r = real_(gen_); return mn + (r * (mx - mn)); }
	int RandInt(int mn, int mx) { if (mn == mx) return mn; int r = int_(gen_); return mn + r % (mx - mn); }
	bool FlipCoin() { return RandDouble(0, 1) < 0.5; }
	int RandSign() { return FlipCoin() ? -1 : 1; }
	// the engine's state as text (the distributions keep none between draws: every draw above is one engine call)
	std::string State() const { std::ostringstream os; os << gen_; return os.str(); }
	bool SetState(const char* txt) { std::istringstream is(txt); std::default_random_engine g; is >> g; if (is.fail()) return false; gen_ = g; real_.reset(); int_.reset(); return true; }
private:
	std::default_random_engine gen_;
	std::uniform_real_distribution<double> real_{0, 1};
	std::uniform_int_distribution<int> int_{0, std::numeric_limits<int>::max()};
};

enum TerrainType { kTerrFlat, kTerrGaps, kTerrSteps, kTerrWalls, kTerrBumps, kTerrMixed, kTerrNarrowGaps, kTerrSlopes, kTerrSlopesGaps,
	kTerrSlopesSteps, kTerrSlopesWalls, kTerrSlopesMixed, kTerrSlopesNarrowGaps, kTerrCliffs, kTerrTypeMax };
constexpr int kNumTerrainParams = 40;
extern const char* const kTerrainTypeNames[kTerrTypeMax];
extern const char* const kTerrainParamNames[kNumTerrainParams];
extern const double kTerrainParamDefaults[kNumTerrainParams];

// appends one terrain strip of (at least) `width` metres to `out`; returns the width added (cTerrainGen2D::tTerrainFunc)
double BuildTerrain(int type, double width, const double* params, TerrainRand& rand, std::vector<float>& out);

// Everything of a GroundWindow that decides which segments it holds and which it builds NEXT (cGroundVar2D's mSegments, mFlipSeg and its cRand, sim/GroundVar2D.cpp):
// both segments in storage order, the flip flag, the build count and the generator's state (its textual form: operator<< of the standard engine). The terrain
// type and parameters are batch settings and stay out. Plain data: part of an env snapshot's host payload (dtrl_engine.h Snapshot).
struct GroundWindowState {
	double min_x[2], origin_x[2], scale_x[2];
	int64_t builds;
	int32_t n[2];
	int32_t flip, pad_;
	char rng[64];
	float data[2][kSegCap];
};
// cGroundVar2D: two sliding heightfield segments of one env, host-resident mirror of the device GroundRec
class GroundWindow {
public:
	bool SaveState(GroundWindowState& out) const;   // false: a segment exceeds kSegCap vertices
	bool LoadState(const GroundWindowState& in);    // false: malformed record (vertex counts, generator state)
	void Configure(int type, const double* params, double world_scale, double segment_width);
	void SetParams(const double* params);
	// another terrain for the segments built from now on (terrain sets: dtrl_assign_terrains); like SetParams it leaves the built segments and the generator alone
	void SetTerrain(int type, const double* params) { type_ = type; SetParams(params); }
	void ResetBuilds() { builds_ = 0; }
	void SeedRand(unsigned long seed) { rand_.Seed(seed); }
	void Clear();
	// returns true when a segment was (re)built, i.e. the device record must be refreshed
	bool Update(double bound_min_x, double bound_max_x);   // sim/GroundVar2D.cpp:43-91
	bool NeedsUpdate(double bound_min_x, double bound_max_x) const;   // Update() would (re)build a segment
	void InitSegments(double bound_min_x, double bound_max_x);
	bool FillRecord(GroundRec& rec, std::string& err) const;
	long num_builds() const { return builds_; }
private:
	struct Seg { std::vector<float> data; double min_x = 0, origin_x = 0, scale_x = 0.1; double MaxX() const; double MinX() const; };
	void BuildSegment(int seg_id, double bound_min, double bound_max, bool align_min, double fix_y);
	int SegID(int s) const { return flip_ ? (s == 0 ? 1 : 0) : s; }
	int type_ = 0; double params_[kNumTerrainParams]; double world_scale_ = 1, segment_width_ = 20;
	TerrainRand rand_;
	Seg segs_[2];
	bool flip_ = false;
	long builds_ = 0;
};

// ---- scenario configuration flattened from the arg file + data files ----
struct ScenarioConfig {
	DevModel model{};
	ModelScalarsD scalars{};       // the character file's doubles behind model.mass / inertia / kp / kd / torque_lim (dtrl_types.h): the base values of the variant rescale
	RunParams run{};
	NetDesc net{};
	bool has_policy_net = false;
	// CACLA (sim/BaseControllerCacla.cpp): the policy net is the ACTOR alone (slice / 3 conv / terr_ip0 / ip1 / ip2 / output). It runs on the
	// device as a MACE-family net with one fragment whose critic head is all zeros; the boundary keeps the actor's own sizes and blob order
	bool actor_only = false;
	int64_t user_num_params = 0;   // what dtrl_set_policy expects (== net.num_params unless actor_only)
	int user_out_size = 0;         // normaliser length at the boundary (== net.out_size unless actor_only)
	int terrain_type = 0;
	std::vector<std::vector<double>> terrain_param_sets;
	double terrain_blend = 0;
	uint64_t terrain_seed = 0;
	bool external_policy = false;  // -policy_mode= external: envs park at their decisions and the caller supplies the actions (dtrl_pending_actions / dtrl_supply_actions)
	std::string char_ctrl;         // the controller's name as given (messages)
	bool device_terrain = false;   // -terrain_gen= device: windows are generated and slid by the GPU at the frame boundary (dtrl_terrain_dev.h)
	int tuple_buffer_size = 16;
	bool tuple_ring_host = false;  // -tuple_ring= host: the tuple rings live in page-locked host memory the kernels write directly (drains without a device copy)
	int tuple_ring_capacity = 0;   // -tuple_ring_capacity=: rows of the device tuple ring (0 = max(2 num_envs, tuple_buffer_size))
	// cScenarioSimChar::ApplyRandForce ranges (scenarios/ScenarioSimChar.cpp:60-63, 88-91; the duration key's typo is the reference's)
	double min_perturb = 50, max_perturb = 100, min_perturb_duration = 0.1, max_perturb_duration = 0.5;
	std::string data_root;
	std::string policy_net_file, policy_model_file;
};

// chr (model variants, dtrl_variant_load_*): the character description comes from `text` (JSON) instead of the file -character_file= names; `name` stands for
// the file in messages. Everything else -- arguments, controller files, state file, terrain, net -- is read as at creation, so every derived field of the
// variant's DevModel comes out of this one code path.
struct CharSource { std::string name; const std::string* text = nullptr; };
bool LoadScenario(const ArgParser& args, ScenarioConfig& cfg, std::string& err, const CharSource* chr = nullptr);
// -character_file= as LoadScenario resolves it: relative to -data_root=, absolute paths as they are
std::string ResolveDataPath(const std::string& root, const std::string& rel);
bool ParseDeployPrototxt(const std::string& path, NetDesc& d, std::string& err, bool* actor_only = nullptr);
// cBaseControllerMACE::BuildNNOutputOffsetScale + cDogControllerMACE::BuildActorBias
void BuildOutputOffsetScale(const DevModel& m, const NetDesc& d, std::vector<double>& off, std::vector<double>& scale);
void LerpTerrainParams(const ScenarioConfig& cfg, double lerp, double* out);
void LerpTerrainParams(const std::vector<std::vector<double>>& sets, double lerp, double* out);   // the same over any file's parameter sets (terrain sets)
// the terrain-file reader of creation (scenarios/ScenarioSimChar.cpp:670-706, sim/TerrainGen2D.cpp:69-81): "Type" and every 40-vector of "Params" with the
// defaults of kTerrainParamDefaults. 0 = read, 1 = the file cannot be read or parsed, 2 = unknown type name (err set)
int LoadTerrainFile(const std::string& path, int& type, std::vector<std::vector<double>>& sets, std::string& err);
int TerrainTypeByName(const std::string& name);   // "" == flat (cTerrainGen2D::ParseType); -1: unknown

}  // namespace dtrl
