"""The reference's configuration surface (config.py:1-54): every name and
value is kept, so ``from config import *`` code runs unchanged.  Only the
integer dtype of the two action arrays differs in spelling: the reference's
``np.int`` (config.py:21,26) was removed from numpy 1.24 and aliased the
builtin ``int``.  The MI355X build's own knobs are at the end.
"""
import numpy as np

# --- frame colours (RGB) the pixel path matches on -----------------------
BG_COLOUR = (144, 72, 17)
BALL_COLOUR = (236, 236, 236)
LEFT_GUY_COLOUR = (213, 130, 74)
RIGHT_GUY_COLOUR = (92, 186, 92)

# --- playfield: rows GAME_TOP..GAME_BOTTOM of the 210x160 frame -----------
GAME_TOP = 34
GAME_BOTTOM = 194
GAME_PLAYABLE_HEIGHT = GAME_BOTTOM - GAME_TOP   # 160
GAME_WIDTH = 160
SCALED_PADDLE_HEIGHT = 16.0
FPS = 60

# --- the 16-button action vector: right paddle [4:6], left paddle [6:8] ---
RIGHT_ACTION_START = 4
RIGHT_ACTION_END = 6
LEFT_ACTION_END = 8
RIGHT_PLAYER_START_BUTTON = 0
LEFT_PLAYER_START_BUTTON = -1
BLANK_ACTION = np.zeros(shape=(16,), dtype=int)
for _button in (LEFT_PLAYER_START_BUTTON, RIGHT_PLAYER_START_BUTTON):
    BLANK_ACTION[_button] = 1
del _button
N_CLASSES = 2
ALL_ACTIONS = np.eye(N_CLASSES, dtype=int)

# --- episode ---------------------------------------------------------------
TIMEOUT_THRESH = 2_000
WIN_SCORE = 3
TIME_SCALER = 100.0
RENDER = False

# --- policy network --------------------------------------------------------
NETWORK_SHAPE = [6, 2, 2]
BIAS = True

# --- genetic algorithm -----------------------------------------------------
GAUSSIAN_MUTATION_MEAN = 0
GAUSSIAN_MUTATION_SIGMA = 0.9
GAUSSIAN_MUTATION_PROBABILITY = 0.9
PROBABILITY_OF_MUTATING_A_SINGLE_GENE = 0.9
CROSSOVER_BLEND_PROBABILITY = 0.9
CROSSOVER_BLEND_ALPHA = 0.9

# often changed
POPULATION_SIZE = 64
GAMES_TO_PLAY = 6
GENERATIONS_BEFORE_SAVE = 5
TOURNAMENT_SIZE = POPULATION_SIZE // 4
HALL_OF_FAME_AMOUNT = TOURNAMENT_SIZE

# --- MI355X build knobs (new; the reference has no device/precision/seed) ---
# Base seed of the Pong physics' serve randomness, per game slot (DESIGN.md "Physics").
PHYSICS_SEED = 0
# "certified": f32 hidden math whose f64 argmax is proven per decision (f64
# re-decision otherwise); "f64": numpy_nn's f64 arithmetic for every pass.
PRECISION = "certified"
# The networks' activation_function (the reference selects it with one line,
# numpy_nn.py:26): "sigmoid" (numpy_nn.py:22-23) or "relu" (numpy_nn.py:6-9, the
# "alternative activation function"), applied to every layer.  The drop-in
# numpy_nn.activation_function starts from it.
ACTIVATION = "sigmoid"
# The evaluation kernel (pong_amd.device.KERNELS): "auto" picks by shape,
# activation and precision.  "relu_wide" is the opt-in for wide ReLU networks
# (ACTIVATION = "relu", NETWORK_SHAPE [6, 2..512, 2..512, 2..4]), which "auto"
# leaves on the general kernel; "sig2" is the opt-in certified f32 kernel for
# two-hidden-layer sigmoid networks (ACTIVATION = "sigmoid", NETWORK_SHAPE
# [6, 2..64, 2..64, 2..4], BIAS), which "auto" leaves on the general kernel (on
# the wide one from 64 units up); "relu2_block" is the opt-in certified f32
# kernel for two-hidden-layer ReLU networks of up to 128 units a layer
# (ACTIVATION = "relu", NETWORK_SHAPE [6, 2..128, 2..128, 2..4], BIAS), which
# "auto" leaves on the general kernel above 64 units (it takes
# no "+advance" or "+solo"); "sig2_block" is the same for sigmoid networks
# (ACTIVATION = "sigmoid", the same shapes, BIAS), which "auto" runs on the
# wide kernel from 64 units up (no "+advance" or "+solo"
# either); "relu3" is the opt-in certified f32 kernel for three-hidden-layer
# ReLU networks (ACTIVATION = "relu", NETWORK_SHAPE [6, 2..32, 2..32, 2..32,
# 2..4], BIAS), which "auto" leaves on the general kernel (it
# takes "+advance" and "+solo" as "relu2" does); "sig3" is the same for
# three-hidden-layer sigmoid networks (ACTIVATION = "sigmoid", the same shapes,
# BIAS), which "auto" leaves on the general kernel too (DESIGN.md 4.2n;
# "sig3+advance", "sig3+solo" and both, as "sig2" takes them); a kernel that cannot run the configured
# network is an error, never a fallback.  "relu+advance", "relu2+advance",
# "sig2+advance" and "auto+advance" are the opt-in closed-form frame advance of
# the certified f32 kernels (serve delays and periodic rallies are not stepped
# frame by frame; the same results); "auto+advance" picks as
# "auto" does and advances where that is the relu or the relu2 kernel.
# "+solo" on the same four names ("relu+solo", "relu2+solo", "sig2+solo",
# "auto+solo"; with the advance "auto+advance+solo", in either order) plays the
# games against the scripted opponents -- evaluate()'s first three, and all of
# generation 0 -- on half a lane group each (the same results).
KERNEL = "auto"
# Storage type of genomes on the device; float64 keeps Python floats exact.
GENOME_DTYPE = "float64"
# "cuda" = the process's current HIP device (one process per GPU).
DEVICE = "cuda"
# evaluate(render=True) writes each replayed game here as game_<g>.gif (no viewer window).
REPLAY_DIR = "replays"
