// A/B table (round 4): block 3 (192 -> 224) variants at 3-sample tiles
#define APNEAUQ_X3_LAYERS(X)                     \
  X(1, 128, 192, 5, 4, 2, 4, false, -8, 0, 32, 1, false) \
  X(2, 192, 224, 3, 3, 1, 7, false, 1, 1, 64, 1, false) \
  X(3, 224, 96, 7, 4, 2, 2, false, 4, 4, 32, 1, false)  \
  X(4, 96, 256, 9, 2, 1, 8, false, 4, 4, 32, 1, false)  \
  X(5, 256, 96, 9, 4, 2, 2, true, 4, 4, 64, 1, false)
